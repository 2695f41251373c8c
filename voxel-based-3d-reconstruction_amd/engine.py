"""CarveEngine: Python face of one libvoxcarve context (one GPU, one z-slab of the grid).

Array-shaped fast path of the reference's carve step:
voxel_reconstruction.py:35-124 + assignment.py:116-133.  All compute happens in the HIP
library; this class only marshals numpy buffers across the C ABI.
"""
import ctypes
import sys

import numpy as np

from . import _lib, lighting
from .camera import Camera

# reference voxel_reconstruction.py:35-36 (x_min, x_max, y_min, y_max, z_min, z_max)
DEFAULT_BOUNDS = (-512.0, 1024.0, -1024.0, 1024.0, -2048.0, 512.0)
SCALING_FACTOR = 64          # reference assignment.py:118
COLOR_CAMERA_INDEX = 1       # reference assignment.py:133 uses camera key 2 (1-based)

MODES = {"fused": _lib.VC_MODE_FUSED, "lut": _lib.VC_MODE_LUT}
FOOTPRINTS = ("centre", "any", "all")


def footprint_rule(footprint):
    """"centre" -> None; "any" | "all" | ("cover", q), q an integer in 1..256 -> (rule, q) of vc_carve_footprint."""
    if isinstance(footprint, str):
        if footprint == "centre":
            return None
        if footprint == "any":
            return (_lib.VC_FOOT_ANY, 0)
        if footprint == "all":
            return (_lib.VC_FOOT_COVER, 256)
    elif isinstance(footprint, (tuple, list)) and len(footprint) == 2 and footprint[0] == "cover":
        q = footprint[1]
        if isinstance(q, (int, np.integer)) and not isinstance(q, bool) and 1 <= int(q) <= 256:
            return (_lib.VC_FOOT_COVER, int(q))
    raise ValueError('footprint %r, expected "centre", "any", "all" or ("cover", q) with an integer q in 1..256' % (footprint,))


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _stats(st, **overrides):
    """A filled Vc*Stats struct as a dict, field by field of its _fields_: integers as int, the *_ms floats as float, arrays as
    a tuple of int.  `overrides` replace or add keys: what a pass reports differently from its struct, said at the call."""
    out = {}
    for name, ctype in st._fields_:
        v = getattr(st, name)
        out[name] = tuple(int(x) for x in v) if isinstance(v, ctypes.Array) else float(v) if ctype is ctypes.c_float else int(v)
    out.update(overrides)
    return out


class CarveEngine:
    def __init__(self, device=0):
        self._L = _lib.load()
        self._ctx = _lib.c_ctx()
        _lib.check(self._L.vc_create(int(device), ctypes.byref(self._ctx)), None, "vc_create")
        self.device = device
        self.grid = None
        self.slab = None
        self.n_cameras = 0
        self.image_size = None
        self.count = 0
        self.n_ranks, self.rank = 1, 0
        self._cams = []                      # what set_cameras() was given
        self._pin_bytes = 0                  # the page-locked buffer of fetch_records(pinned=True)
        # the sizes of the last pass's outputs, which its fetch_* calls allocate by: empty until the pass has run
        self._render_shape = (0, (0, 0))     # views and size of the last render()
        self._mesh_verts = 0                 # vertices of the last surface_mesh()
        self._photo_n = 0                    # records the last photo_carve() started from
        self._cc_n, self._cc_k = 0, 0        # records the last filter_components() started from, and its components
        self._cl_k = 0                       # figures of the last cluster_hull()
        self._geo_k = 0                      # extremities of the last hull_geodesic()
        self._ms_g = 0                       # groups of the last measure_hull()
        self._shell_t = 0                    # cells of the last hull_shell()
        self._thin = (0, 0)                  # records the last thin_hull() started from, and the voxels it kept
        self._motion = (8, 4, 4)             # block, apron and search of the last hull_motion()

    # -- lifetime -----------------------------------------------------------------
    def close(self):
        if self._ctx:
            self._release_pinned()
            self._L.vc_destroy(self._ctx)
            self._ctx = _lib.c_ctx()

    def __del__(self):
        # an engine that is still alive when the interpreter shuts down (a module's global, such as
        # background_subtraction._engine) is left to the process's exit: its context's teardown would run inside a finalising
        # interpreter, beside the exit handlers of whatever else holds a HIP runtime in the process (torch brings its own copy)
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        _lib.check(rc, self._ctx, what)

    # -- geometry -----------------------------------------------------------------
    def set_grid(self, nx, ny, nz, bounds=DEFAULT_BOUNDS):
        b = np.asarray(bounds, dtype=np.float64).reshape(6)
        self._check(self._L.vc_set_grid(self._ctx, nx, ny, nz, _ptr(b, ctypes.c_double)), "vc_set_grid")
        self.grid = (int(nx), int(ny), int(nz))
        self.bounds = tuple(float(v) for v in b)
        self.slab = (0, int(nz))

    def set_slab(self, z0, z1):
        self._check(self._L.vc_set_slab(self._ctx, z0, z1), "vc_set_slab")
        self.slab = (int(z0), int(z1))

    @property
    def n_voxels(self):
        nx, ny, _ = self.grid
        return nx * ny * (self.slab[1] - self.slab[0])

    @property
    def index_base(self):
        nx, ny, _ = self.grid
        return self.slab[0] * nx * ny

    def axes(self):
        nx, ny, nz = self.grid
        xs, ys, zs = np.empty(nx), np.empty(ny), np.empty(nz)
        self._check(self._L.vc_get_axes(self._ctx, _ptr(xs, ctypes.c_double), _ptr(ys, ctypes.c_double),
                                        _ptr(zs, ctypes.c_double)), "vc_get_axes")
        return xs, ys, zs

    # -- cameras ------------------------------------------------------------------
    def set_cameras(self, cameras, H, W):
        cams = [c if isinstance(c, Camera) else Camera(*c) for c in cameras]
        K9 = np.ascontiguousarray([c.K.reshape(9) for c in cams], dtype=np.float64)
        d5 = np.ascontiguousarray([c.dist for c in cams], dtype=np.float64)
        R9 = np.ascontiguousarray([c.R.reshape(9) for c in cams], dtype=np.float64)
        t3 = np.ascontiguousarray([c.tvec for c in cams], dtype=np.float64)
        dp = ctypes.c_double
        self._check(self._L.vc_set_cameras(self._ctx, len(cams), _ptr(K9, dp), _ptr(d5, dp), _ptr(R9, dp),
                                           _ptr(t3, dp), H, W), "vc_set_cameras")
        self.n_cameras = len(cams)
        self._cams = cams
        self.image_size = (int(H), int(W))

    @property
    def cameras(self):
        """The camera.Camera list of the last set_cameras (the calibrated cameras): read-only."""
        return self._cams

    # -- per-frame inputs -----------------------------------------------------------
    def upload_masks(self, masks, slot=0):
        m = np.ascontiguousarray(np.stack([np.asarray(x) for x in masks]), dtype=np.uint8)
        if m.shape != (self.n_cameras,) + self.image_size:
            raise ValueError("masks shape %s, expected %s" % (m.shape, (self.n_cameras,) + self.image_size))
        self._check(self._L.vc_upload_masks(self._ctx, slot, _ptr(m, ctypes.c_uint8)), "vc_upload_masks")

    def touch_masks(self, slot=0):
        """Treat the slot's resident byte masks / images as new input: the next carve re-derives bit masks, block
        grids and camera order from them on the device (no transfer)."""
        self._check(self._L.vc_touch_masks(self._ctx, slot), "vc_touch_masks")

    def set_mask_postfilter(self, open2x2=None, close2x2=None):
        """Per-camera 2x2 MORPH_OPEN / MORPH_CLOSE applied on the device to every following
        upload_masks (tail of the reference's extract_foreground_mask, background_subtraction.py:195-206)."""
        def arr(flags):
            if flags is None:
                return None
            a = np.ascontiguousarray([1 if f else 0 for f in flags], dtype=np.uint8)
            if a.size != self.n_cameras:
                raise ValueError("need one flag per camera")
            return a
        o, c = arr(open2x2), arr(close2x2)
        self._check(self._L.vc_set_mask_postfilter(self._ctx, _ptr(o, ctypes.c_uint8) if o is not None else None,
                                                   _ptr(c, ctypes.c_uint8) if c is not None else None), "vc_set_mask_postfilter")

    # -- the step before the path: data-parallel part of extract_foreground_mask --------------------------------
    def bgr_to_hsv(self, image):
        """cv2.cvtColor(image, cv2.COLOR_BGR2HSV) on uint8 [H,W,3], on the device (background_subtraction.py:155)."""
        a = np.ascontiguousarray(image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image shape %s, expected [H, W, 3]" % (a.shape,))
        out = np.empty_like(a)
        self._check(self._L.vc_bgr_to_hsv(self._ctx, _ptr(a, ctypes.c_uint8), a.shape[0], a.shape[1], _ptr(out, ctypes.c_uint8)), "vc_bgr_to_hsv")
        return out

    def mask_morphology(self, mask, ksize, opening=False, closing=False):
        """cv2.morphologyEx with a ksize x ksize MORPH_RECT element on uint8 [H,W]: MORPH_OPEN, then MORPH_CLOSE, as asked
        (background_subtraction.py:161-168 with ksize 3, :195-203 with ksize 2)."""
        a = np.ascontiguousarray(mask, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("mask shape %s, expected [H, W]" % (a.shape,))
        out = np.empty_like(a)
        self._check(self._L.vc_mask_morphology(self._ctx, _ptr(a, ctypes.c_uint8), a.shape[0], a.shape[1], int(ksize), int(bool(opening)),
                                               int(bool(closing)), _ptr(out, ctypes.c_uint8)), "vc_mask_morphology")
        return out

    # ---- the MOG background model (cv2.bgsegm.createBackgroundSubtractorMOG; background_subtraction.py:75-92, :158)
    def mog_create(self, history=200, nmixtures=5, background_ratio=0.7, noise_sigma=0):
        model = ctypes.c_uint32(0)
        self._check(self._L.vc_mog_create(self._ctx, int(history), int(nmixtures), float(background_ratio), float(noise_sigma),
                                          ctypes.byref(model)), "vc_mog_create")
        return model.value

    def mog_apply(self, model, image, learning_rate=-1):
        a = np.ascontiguousarray(image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image shape %s, expected [H, W, 3]" % (a.shape,))
        out = np.empty(a.shape[:2], dtype=np.uint8)
        self._check(self._L.vc_mog_apply(self._ctx, int(model), _ptr(a, ctypes.c_uint8), a.shape[0], a.shape[1], float(learning_rate),
                                         _ptr(out, ctypes.c_uint8)), "vc_mog_apply")
        return out

    def mog_state(self, model):
        """(state float32 [8 nmixtures, H W] planes -- plane 8 k + f: field f (sort key, weight, mean[3], var[3]) of component k --,
        (H, W), frames seen)."""
        H, W, K, nf = (ctypes.c_uint32(0) for _ in range(4))
        self._check(self._L.vc_mog_state(self._ctx, int(model), None, 0, ctypes.byref(H), ctypes.byref(W), ctypes.byref(K), ctypes.byref(nf)),
                    "vc_mog_state")
        state = np.zeros((8 * K.value, H.value * W.value), dtype=np.float32)
        if state.size:
            self._check(self._L.vc_mog_state(self._ctx, int(model), _ptr(state, ctypes.c_float), state.size, None, None, None, None), "vc_mog_state")
        return state, (H.value, W.value), nf.value

    def foreground_front(self, model, image, learning_rate=0, opening=False, closing=False, to_hsv=True):
        """BGR -> HSV, the model's apply, 3x3 open / close: extract_foreground_mask up to its contour stage, one call
        (background_subtraction.py:155-168)."""
        a = np.ascontiguousarray(image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image shape %s, expected [H, W, 3]" % (a.shape,))
        out = np.empty(a.shape[:2], dtype=np.uint8)
        self._check(self._L.vc_foreground_front(self._ctx, int(model), _ptr(a, ctypes.c_uint8), a.shape[0], a.shape[1], int(bool(to_hsv)),
                                                float(learning_rate), int(bool(opening)), int(bool(closing)), _ptr(out, ctypes.c_uint8)),
                    "vc_foreground_front")
        return out

    def fill_figures(self, mask, figure_threshold, figure_inner_threshold):
        """The contour stage of extract_foreground_mask (background_subtraction.py:171-193) on the device: contours of area
        >= figure_threshold filled, their children of oriented area >= figure_inner_threshold cleared with the outline kept.
        uint8 [H, W] (foreground where != 0) in, uint8 [H, W] {0, 255} out."""
        a = np.ascontiguousarray(mask, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("mask shape %s, expected [H, W]" % (a.shape,))
        out = np.empty(a.shape, dtype=np.uint8)
        self._check(self._L.vc_fill_figures(self._ctx, _ptr(a, ctypes.c_uint8), a.shape[0], a.shape[1], float(figure_threshold),
                                            float(figure_inner_threshold), _ptr(out, ctypes.c_uint8)), "vc_fill_figures")
        return out

    def foreground_to_slot(self, models, frames, params, slot=0, learning_rate=0):
        """extract_foreground_mask of every camera's BGR frame straight into carve slot `slot` (background_subtraction.py:129-208
        as assignment.py:98-109 calls it), the frames becoming the slot's images.  models: one background model per camera
        (BackgroundSubtractorMOG / BackgroundSubtractorMOG2 of this engine, or a model handle; the kinds may be mixed); params:
        per camera [figure_threshold, figure_inner_threshold, opening_pre, closing_pre, ...] (the rows of
        assignment.cam_bg_model_params).  The 2x2 post-filter is set_mask_postfilter's.
        Asynchronous: the next carve on the slot waits for it on the device."""
        ids = np.array([int(m if isinstance(m, (int, np.integer)) else m._model) for m in models], dtype=np.uint32)
        f = np.ascontiguousarray(np.stack([np.asarray(x) for x in frames]), dtype=np.uint8)
        if f.ndim != 4 or f.shape[3] != 3:
            raise ValueError("frames shape %s, expected [C, H, W, 3]" % (f.shape,))
        n = f.shape[0]
        if n != self.n_cameras or len(params) < n:
            raise ValueError("%d frames and %d parameter rows for %d cameras" % (n, len(params), self.n_cameras))
        ft = np.array([float(params[c][0]) for c in range(n)], dtype=np.float64)
        it = np.array([float(params[c][1]) for c in range(n)], dtype=np.float64)
        op = np.array([bool(params[c][2]) for c in range(n)], dtype=np.uint8)
        cl = np.array([bool(params[c][3]) for c in range(n)], dtype=np.uint8)
        self._check(self._L.vc_foreground_to_slot(self._ctx, slot, _ptr(ids, ctypes.c_uint32), len(ids), _ptr(f, ctypes.c_uint8),
                                                  f.shape[1], f.shape[2], float(learning_rate), _ptr(ft, ctypes.c_double),
                                                  _ptr(it, ctypes.c_double), _ptr(op, ctypes.c_uint8), _ptr(cl, ctypes.c_uint8)),
                    "vc_foreground_to_slot")

    def mog_destroy(self, model):
        self._check(self._L.vc_mog_destroy(self._ctx, int(model)), "vc_mog_destroy")

    # ---- the MOG2 background model (cv2.createBackgroundSubtractorMOG2; background_subtraction.py:90-127, :158)
    def mog2_create(self, history=500, var_threshold=16, detect_shadows=True, nmixtures=5, background_ratio=0.9, var_threshold_gen=9,
                    var_init=15, var_min=4, var_max=75, complexity_reduction_threshold=0.05, shadow_value=127, shadow_threshold=0.5):
        """A MOG2 model on this device; returns its handle (VC_MOG2_MODEL_TAG | index).  nmixtures: 1..8."""
        model = ctypes.c_uint32(0)
        self._check(self._L.vc_mog2_create(self._ctx, int(history), float(var_threshold), int(bool(detect_shadows)), int(nmixtures),
                                           float(background_ratio), float(var_threshold_gen), float(var_init), float(var_min),
                                           float(var_max), float(complexity_reduction_threshold), int(shadow_value),
                                           float(shadow_threshold), ctypes.byref(model)), "vc_mog2_create")
        return model.value

    def mog2_apply(self, model, image, learning_rate=-1):
        a = np.ascontiguousarray(image, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image shape %s, expected [H, W, 3]" % (a.shape,))
        out = np.empty(a.shape[:2], dtype=np.uint8)
        self._check(self._L.vc_mog2_apply(self._ctx, int(model), _ptr(a, ctypes.c_uint8), a.shape[0], a.shape[1], float(learning_rate),
                                          _ptr(out, ctypes.c_uint8)), "vc_mog2_apply")
        return out

    def mog2_state(self, model):
        """(state float32 [5 nmixtures, H W] planes -- plane 5 k + f: field f (weight, variance, mean[3]) of component k --,
        nmodes uint8 [H W], (H, W), frames seen)."""
        H, W, K, nf = (ctypes.c_uint32(0) for _ in range(4))
        self._check(self._L.vc_mog2_state(self._ctx, int(model), None, 0, None, 0, ctypes.byref(H), ctypes.byref(W), ctypes.byref(K),
                                          ctypes.byref(nf)), "vc_mog2_state")
        state = np.zeros((5 * K.value, H.value * W.value), dtype=np.float32)
        nmodes = np.zeros(H.value * W.value, dtype=np.uint8)
        if nmodes.size:
            self._check(self._L.vc_mog2_state(self._ctx, int(model), _ptr(state, ctypes.c_float), state.size, _ptr(nmodes, ctypes.c_uint8),
                                              nmodes.size, None, None, None, None), "vc_mog2_state")
        return state, nmodes, (H.value, W.value), nf.value

    def mog2_destroy(self, model):
        self._check(self._L.vc_mog2_destroy(self._ctx, int(model)), "vc_mog2_destroy")

    def fetch_mask(self, cam, slot=0):
        out = np.empty(self.image_size, dtype=np.uint8)
        self._check(self._L.vc_fetch_mask(self._ctx, slot, cam, _ptr(out, ctypes.c_uint8)), "vc_fetch_mask")
        return out

    def upload_frame(self, cam, bgr, slot=0):
        f = np.ascontiguousarray(bgr, dtype=np.uint8)
        if f.shape != self.image_size + (3,):
            raise ValueError("frame shape %s, expected %s" % (f.shape, self.image_size + (3,)))
        self._check(self._L.vc_upload_frame(self._ctx, slot, cam, _ptr(f, ctypes.c_uint8)), "vc_upload_frame")

    # -- lookup table ---------------------------------------------------------------
    def build_lut(self):
        self._check(self._L.vc_build_lut(self._ctx), "vc_build_lut")

    def fetch_lut(self, cam):
        out = np.empty(self.n_voxels, dtype=np.int32)
        self._check(self._L.vc_fetch_lut(self._ctx, cam, _ptr(out, ctypes.c_int32)), "vc_fetch_lut")
        return out

    # -- lookup-table persistence (reference: the pickled table of assignment.py:12-15; here a .npz, nothing executable) ----
    def _lut_meta(self):
        import hashlib
        h = hashlib.sha256()
        for c in self._cams:
            for a in (c.K, c.dist, c.R, c.tvec):
                h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        return {"format": "voxcarve-lut-1", "grid": list(self.grid), "slab": list(self.slab), "bounds": list(self.bounds),
                "image_size": list(self.image_size), "cameras": self.n_cameras, "cameras_sha256": h.hexdigest(),
                "entry": "int32 pixel offset int(v) * W + int(u) of the voxel's projection, -1 outside the image "
                         "(voxel_reconstruction.py:110-112); voxel order i = iz*nx*ny + ix*ny + iy of the slab"}

    def save_lut(self, path):
        """Writes the packed table of this context (grid, slab, cameras) as <path> (.npz: 'lut' int32 [C, n] + 'meta' JSON)."""
        import json
        lut = np.stack([self.fetch_lut(c) for c in range(self.n_cameras)])
        with open(path, "wb") as f:
            np.savez(f, lut=lut, meta=np.frombuffer(json.dumps(self._lut_meta()).encode(), dtype=np.uint8))

    def load_lut(self, path):
        """Hands a table written by save_lut to the device instead of projecting it again.  The file must have been made
        for exactly this grid, slab, bounds, mask size and these cameras: anything else raises VoxcarveError."""
        import json
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(bytes(z["meta"]).decode())
            want = self._lut_meta()
            bad = [k for k in want if k != "entry" and meta.get(k) != want[k]]
            if bad:
                raise _lib.VoxcarveError("lookup table %s was made for another configuration (differs in: %s)" % (path, ", ".join(bad)))
            lut = z["lut"]
            if lut.dtype != np.int32 or lut.shape != (self.n_cameras, self.n_voxels):
                raise _lib.VoxcarveError("lookup table %s: array %s %s, expected int32 %s" % (path, lut.dtype, lut.shape, (self.n_cameras, self.n_voxels)))
            hw = int(self.image_size[0]) * int(self.image_size[1])            # (equal to the file's: checked above)
            lo, hi = (int(lut.min()), int(lut.max())) if lut.size else (-1, -1)
            if lo < -1 or hi >= hw:
                raise _lib.VoxcarveError("lookup table %s holds entries outside [-1, H*W) (min %d, max %d): stale or corrupt file" % (path, lo, hi))
            self.upload_lut(lut)

    def upload_lut(self, lut):
        """int32 [C, n] in voxel order (what fetch_lut gives out per camera); adopted once all cameras are in."""
        lut = np.ascontiguousarray(lut, dtype=np.int32)
        if lut.shape != (self.n_cameras, self.n_voxels):
            raise ValueError("lut shape %s, expected %s" % (lut.shape, (self.n_cameras, self.n_voxels)))
        for c in range(self.n_cameras):
            self._check(self._L.vc_upload_lut(self._ctx, c, _ptr(lut[c], ctypes.c_int32)), "vc_upload_lut")

    def project(self, cam, points):
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        uv = np.empty((p.shape[0], 2), dtype=np.float64)
        self._check(self._L.vc_project(self._ctx, cam, _ptr(p, ctypes.c_double), p.shape[0],
                                       _ptr(uv, ctypes.c_double)), "vc_project")
        return uv

    # -- hot path -------------------------------------------------------------------
    def carve(self, slot=0, min_views=None, color_cam=COLOR_CAMERA_INDEX, mode="fused", viewmask=False, records=True,
              footprint="centre"):
        """Runs the carve; returns the survivor count (records stay on the device).  records=False keeps
        only the count and the occupancy words (multi-GPU ranks: allgather() / expand_entries() make the list).
        footprint: "centre" (default, the reference's rule: the pixel under the voxel's centre), or a test of the pixel box
        the voxel's whole cell projects to -- "any" (outer hull: some pixel is foreground), "all" (inner hull: the box lies
        in the image and is all foreground), ("cover", q) (at least q / 256 of it); see vc_carve_footprint.  `mode` does
        not apply to those: they project in the kernel."""
        n = ctypes.c_uint64(0)
        mv = self.n_cameras if min_views is None else int(min_views)
        cc = -1 if color_cam is None else int(color_cam)
        flags = (_lib.VC_FLAG_VIEWMASK if viewmask else 0) | (0 if records else _lib.VC_FLAG_NO_RECORDS)
        foot = footprint_rule(footprint)
        if foot is not None:
            self._check(self._L.vc_carve_footprint(self._ctx, slot, mv, cc, foot[0], foot[1], flags, ctypes.byref(n)), "vc_carve_footprint")
            self.count = int(n.value)
            return self.count
        self._check(self._L.vc_carve(self._ctx, slot, mv, cc, MODES[mode], flags, ctypes.byref(n)), "vc_carve")
        self.count = int(n.value)
        return self.count

    def carve_begin(self, slot=0, min_views=None, color_cam=COLOR_CAMERA_INDEX, mode="fused", viewmask=False,
                    records=True):
        """Enqueue a carve step without waiting (at most two in flight), so the device has the next
        step queued while the host collects this one.  carve_end() completes the oldest step."""
        mv = self.n_cameras if min_views is None else int(min_views)
        cc = -1 if color_cam is None else int(color_cam)
        flags = (_lib.VC_FLAG_VIEWMASK if viewmask else 0) | (0 if records else _lib.VC_FLAG_NO_RECORDS)
        self._check(self._L.vc_carve_begin(self._ctx, slot, mv, cc, MODES[mode], flags), "vc_carve_begin")

    def carve_end(self):
        n = ctypes.c_uint64(0)
        self._check(self._L.vc_carve_end(self._ctx, ctypes.byref(n)), "vc_carve_end")
        self.count = int(n.value)
        return self.count

    def fetch(self):
        """(idx u32 [S] ascending global linear index, rgb u8 [S,3], seen bool [S])."""
        S = self.count
        idx = np.empty(S, dtype=np.uint32)
        rgb = np.empty((S, 3), dtype=np.uint8)
        seen = np.empty(S, dtype=np.uint8)
        self._check(self._L.vc_fetch(self._ctx, _ptr(idx, ctypes.c_uint32), _ptr(rgb, ctypes.c_uint8),
                                     _ptr(seen, ctypes.c_uint8)), "vc_fetch")
        return idx, rgb, seen.astype(bool)

    def fetch_records(self, pinned=False):
        """u64 records of the last carve.  pinned=True returns a view of a page-locked buffer
        owned by the engine (valid until the next pinned fetch): PCIe-rate read-back."""
        if not pinned:
            rec = np.empty(self.count, dtype=np.uint64)
            self._check(self._L.vc_fetch_records(self._ctx, _ptr(rec, ctypes.c_uint64)), "vc_fetch_records")
            return rec
        need = max(self.count, 1) * 8
        if self._pin_bytes < need:
            self._release_pinned()
            ptr = ctypes.c_void_p()
            grow = (need + need // 4 + 7) // 8 * 8
            self._check(self._L.vc_host_alloc(self._ctx, grow, ctypes.byref(ptr)), "vc_host_alloc")
            self._pin_ptr, self._pin_bytes = ptr, grow
            self._pin_arr = np.frombuffer((ctypes.c_uint8 * grow).from_address(ptr.value), dtype=np.uint64)
        out = self._pin_arr[:self.count]
        self._check(self._L.vc_fetch_records(self._ctx, _ptr(out, ctypes.c_uint64)), "vc_fetch_records")
        return out

    def _release_pinned(self):
        if self._pin_bytes:
            self._pin_arr = None
            self._L.vc_host_free(self._ctx, self._pin_ptr)
            self._pin_bytes = 0

    def fetch_viewmask(self):
        vm = np.empty(self.n_voxels, dtype=np.uint16)
        self._check(self._L.vc_fetch_viewmask(self._ctx, _ptr(vm, ctypes.c_uint16)), "vc_fetch_viewmask")
        return vm

    def fetch_occupancy(self):
        """Dense survivor bits of the slab: bool [n] (slab-local voxel order)."""
        n = self.n_voxels
        raw = np.empty(((n + 63) // 64) * 8, dtype=np.uint8)
        self._check(self._L.vc_fetch_occupancy(self._ctx, _ptr(raw, ctypes.c_uint8)), "vc_fetch_occupancy")
        return np.unpackbits(raw, bitorder="little")[:n].astype(bool)

    # -- occlusion-aware colouring (vc_color_visible) ----------------------------------------------------------------------------
    def default_depth_tolerance(self):
        """The voxel diagonal as float32: sqrt((2hx)^2 + (2hy)^2 + (2hz)^2), h = half the grid step (0 on an axis of one voxel)."""
        h = [((self.bounds[2 * a + 1] - self.bounds[2 * a]) / (n - 1)) / 2 if n > 1 else 0.0 for a, n in enumerate(self.grid)]
        return float(np.float32(np.sqrt((2 * h[0]) ** 2 + (2 * h[1]) ** 2 + (2 * h[2]) ** 2)))

    def color_visible(self, slot=0, depth_tolerance=None):
        """Recolours the current carve result in place: every surface survivor takes the rounded mean colour of the cameras that
        see it past the per-camera depth maps of the surface voxels (contract: include/voxcarve.h).  Every camera of `slot`
        needs an image.  fetch() / fetch_records() then return the new colours; the next carve the colour camera's again."""
        if depth_tolerance is None:
            depth_tolerance = self.default_depth_tolerance() if self.grid is not None else 0.0   # (no grid: the call reports it)
        tol = float(depth_tolerance)
        self._check(self._L.vc_color_visible(self._ctx, int(slot), tol, 0), "vc_color_visible")

    def fetch_visibility(self):
        """u16 [S] in record order: bit c set = the survivor is visible in camera c (after color_visible)."""
        vis = np.empty(self.count, dtype=np.uint16)
        self._check(self._L.vc_fetch_visibility(self._ctx, _ptr(vis, ctypes.c_uint16)), "vc_fetch_visibility")
        return vis

    def fetch_depth(self, cam):
        """Camera cam's depth map of the surface voxels, float32 [H, W] (+inf where none splatted; after color_visible)."""
        out = np.empty(self.image_size, dtype=np.float32)
        self._check(self._L.vc_fetch_depth(self._ctx, int(cam), _ptr(out, ctypes.c_float)), "vc_fetch_depth")
        return out

    # -- photo-consistency carving (vc_photo_carve) -------------------------------------------------------------------------------
    def photo_carve(self, slot=0, var_threshold=1200, min_views=2, max_rounds=32, depth_tolerance=None):
        """Refines the current carve result by photo-consistency (contract: include/voxcarve.h): rounds of the visibility pass of
        color_visible, every surface voxel whose visible cameras (at least min_views of them) disagree on its colour by more than
        var_threshold (sum of the per-channel variances, squared 8-bit levels) removed, until a round removes nothing or
        max_rounds have run.  Every camera of `slot` needs an image.  The records, the count, the occupancy, the visibility and
        the depth maps then describe the photo hull, coloured as color_visible colours it; the next carve restores the visual
        hull.  Returns the stats as a dict: rounds, converged, survivors_before, survivors_after, photo_ms."""
        if depth_tolerance is None:
            depth_tolerance = self.default_depth_tolerance() if self.grid is not None else 0.0   # (no grid: the call reports it)
        st = _lib.VcPhotoStats()
        self._check(self._L.vc_photo_carve(self._ctx, int(slot), float(depth_tolerance), int(var_threshold), int(min_views),
                                           int(max_rounds), 0, ctypes.byref(st)), "vc_photo_carve")
        self.count = int(st.survivors_after)
        self._photo_n = int(st.survivors_before)
        return _stats(st, converged=bool(st.converged))

    def fetch_photo_rounds(self):
        """u8 [survivors_before]: per record of the last photo_carve's input, in its order, the round that removed it (0 = kept)."""
        out = np.empty(self._photo_n, dtype=np.uint8)
        self._check(self._L.vc_fetch_photo_rounds(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_photo_rounds")
        return out

    # -- connected components of the hull (vc_hull_components) ------------------------------------------------------------------
    def filter_components(self, connectivity=26, min_voxels=0, keep_largest=0):
        """Labels the connected components of the current carve result (face / + edge / + corner neighbours for connectivity 6 /
        18 / 26) and removes the survivors of every component smaller than min_voxels or, when keep_largest > 0, not among the
        keep_largest largest (size descending, then label ascending) -- contract: include/voxcarve.h.  The records, the count
        and the occupancy then describe the kept survivors; the next carve restores the visual hull.  Returns the stats as a
        dict: components, components_kept, survivors_before, survivors_after, largest, components_ms."""
        st = _lib.VcComponentStats()
        self._check(self._L.vc_hull_components(self._ctx, int(connectivity), int(min_voxels), int(keep_largest), 0,
                                               ctypes.byref(st)), "vc_hull_components")
        self.count = int(st.survivors_after)
        self._cc_n, self._cc_k = int(st.survivors_before), int(st.components)
        return _stats(st)

    def fetch_component_labels(self):
        """u32 [survivors_before]: per record of the last filter_components' input, in its order, the label of its component
        (the smallest linear index in it)."""
        out = np.empty(self._cc_n, dtype=np.uint32)
        self._check(self._L.vc_fetch_component_labels(self._ctx, _ptr(out, ctypes.c_uint32)), "vc_fetch_component_labels")
        return out

    def fetch_components(self):
        """The components of the last filter_components in ascending label: dict of numpy arrays label u32 [K], size u32 [K],
        lo / hi u32 [K, 3] (inclusive box in (ix, iy, iz)), kept bool [K]."""
        raw = np.empty((self._cc_k, 10), dtype=np.uint32)
        self._check(self._L.vc_fetch_components(self._ctx, raw.ctypes.data_as(ctypes.c_void_p)), "vc_fetch_components")
        return {"label": raw[:, 0].copy(), "size": raw[:, 1].copy(), "lo": raw[:, 2:5].copy(), "hi": raw[:, 5:8].copy(),
                "kept": raw[:, 8] != 0}

    # -- distance field of the hull, erosion and opening by a ball in mm (vc_hull_distance, vc_hull_morphology) -------------------
    @staticmethod
    def _dist_flags(border, outside=False):
        if border not in ("open", "off"):
            raise ValueError('border %r, expected "open" or "off"' % (border,))
        return (_lib.VC_DIST_BORDER_OFF if border == "off" else 0) | (_lib.VC_DIST_OUTSIDE if outside else 0)

    def hull_distance(self, border="open", outside=False):
        """The exact squared Euclidean distance transform of the current carve result in um^2 (contract: include/voxcarve.h):
        for every survivor the distance to the nearest voxel that is not one (border="off": or to one virtual layer of such
        voxels around the grid) and, with outside=True, for every voxel of the grid the distance to the nearest survivor.  The
        grid steps are rounded to whole micrometres; everything is integer and exact.  Returns the stats as a dict: survivors,
        sites_inside_box, max_d2, q (x, y, z in um), distance_ms.  The fetch_* calls below read the fields."""
        st = _lib.VcDistanceStats()
        self._check(self._L.vc_hull_distance(self._ctx, self._dist_flags(border, outside), ctypes.byref(st)), "vc_hull_distance")
        return _stats(st)

    def fetch_record_distance(self):
        """u64 [S] in record order: the squared inside distance of each survivor in um^2 (after hull_distance, which leaves
        the records alone: S is the current count; the call fails once anything has changed the result)."""
        out = np.empty(self.count, dtype=np.uint64)
        self._check(self._L.vc_fetch_record_distance(self._ctx, _ptr(out, ctypes.c_uint64)), "vc_fetch_record_distance")
        return out

    def fetch_record_depth(self):
        """float64 [S] in record order: how deep inside the hull each survivor lies, in mm (its local half-thickness)."""
        return np.sqrt(self.fetch_record_distance().astype(np.float64)) / 1000

    def fetch_distance_raw(self, which="inside"):
        """u64 [nz, nx, ny]: the dense squared field in um^2, which = "inside" | "outside"; 2^64 - 1 where there is no site."""
        if which not in ("inside", "outside"):
            raise ValueError('which %r, expected "inside" or "outside"' % (which,))
        out = np.empty(self.n_voxels, dtype=np.uint64)
        self._check(self._L.vc_fetch_distance(self._ctx, 1 if which == "outside" else 0, _ptr(out, ctypes.c_uint64)), "vc_fetch_distance")
        nx, ny, nz = self.grid
        return out.reshape(nz, nx, ny)

    def fetch_distance_field(self, which="inside"):
        """float64 [nz, nx, ny] in mm: which = "inside" (depth of the survivors, 0 elsewhere), "outside" (distance to the hull,
        0 on it; needs hull_distance(outside=True)) or "signed" (outside minus inside)."""
        if which == "signed":
            return self.fetch_distance_field("outside") - self.fetch_distance_field("inside")
        return np.sqrt(self.fetch_distance_raw(which).astype(np.float64)) / 1000

    @staticmethod
    def radius_r2(radius_mm):
        """r2 in um^2 of a ball of radius_mm: round(radius_mm * 1000) squared."""
        r = float(radius_mm)
        if not np.isfinite(r) or r < 0:
            raise ValueError("radius %r mm, expected a finite value >= 0" % (radius_mm,))
        r_um = int(round(r * 1000.0))
        return r_um * r_um

    def _morphology(self, op, r2, border):
        if r2 >= 1 << 64:
            raise ValueError("radius^2 = %d um^2 does not fit 64 bits" % r2)
        st = _lib.VcMorphStats()
        self._check(self._L.vc_hull_morphology(self._ctx, op, int(r2), self._dist_flags(border), ctypes.byref(st)), "vc_hull_morphology")
        self.count = int(st.survivors_after)
        return _stats(st)

    def erode_hull(self, radius_mm, border="open"):
        """Erodes the current carve result by a ball of radius_mm millimetres (a Euclidean ball in world units, whatever the grid's
        anisotropy): the survivors whose inside distance is above the radius stay, r2 = round(radius_mm * 1000)^2 um^2.  The
        records, the count and the occupancy then describe the eroded hull; the next carve restores the visual hull.  Returns
        the stats as a dict: survivors_before, eroded, survivors_after, max_d2, q, morph_ms."""
        return self._morphology(_lib.VC_MORPH_ERODE, self.radius_r2(radius_mm), border)

    def open_hull(self, radius_mm, border="open"):
        """Opens the current carve result by a ball of radius_mm millimetres: what is thinner than the ball -- spurs, fins, thin
        bridges and specks of mask noise, attached to the figure or not -- leaves the hull, the rest keeps its shape (the
        survivors within the radius of the eroded set stay).  Arguments, effects and stats as erode_hull."""
        return self._morphology(_lib.VC_MORPH_OPEN, self.radius_r2(radius_mm), border)

    # -- dilation and closing of the hull by a ball in mm (vc_hull_grow): the passes that ADD survivors -----------------------------
    def _grow(self, op, r2):
        if r2 >= 1 << 64:
            raise ValueError("radius^2 = %d um^2 does not fit 64 bits" % r2)
        st = _lib.VcGrowStats()
        self._check(self._L.vc_hull_grow(self._ctx, op, int(r2), 0, ctypes.byref(st)), "vc_hull_grow")
        self.count = int(st.survivors_after)
        return _stats(st)

    def dilate_hull(self, radius_mm):
        """Dilates the current carve result by a ball of radius_mm millimetres (a Euclidean ball in world units, clipped to the
        grid): every voxel within the radius of a survivor becomes one, r2 = round(radius_mm * 1000)^2 um^2.  The records, the
        count and the occupancy then describe the dilated hull: old records keep their bytes, an added voxel is coloured by the
        colour camera's pixel under its centre (contract: include/voxcarve.h).  The next carve restores the visual hull.  Returns
        the stats as a dict: survivors_before, dilated, survivors_after, added, box_cells, q, grow_ms."""
        return self._grow(_lib.VC_GROW_DILATE, self.radius_r2(radius_mm))

    def close_hull(self, radius_mm):
        """Closes the current carve result by a ball of radius_mm millimetres: tunnels, holes and dents narrower than the ball are
        filled -- what a hole in one camera's foreground mask carves through the figure -- and the rest of the hull keeps its
        shape (dilation, then the erosion of the dilated set).  The result holds the hull; closing it again adds nothing.
        Arguments, effects and stats as dilate_hull."""
        return self._grow(_lib.VC_GROW_CLOSE, self.radius_r2(radius_mm))

    def fetch_added(self):
        """u8 [S] in record order: 1 where the record was created by the last dilate_hull / close_hull (fails once a carve or a
        pass that removes survivors has run since)."""
        out = np.empty(self.count, dtype=np.uint8)
        self._check(self._L.vc_fetch_grown(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_grown")
        return out

    # -- the vote over the last frames' hulls (vc_hull_temporal): the one pass whose state outlives a result ------------------------
    @staticmethod
    def temporal_thresholds(window=5, keep=None, keep_off=None):
        """(window, keep_on, keep_off) as temporal_filter takes them: keep defaults to window // 2 + 1 (the majority), keep_off to
        keep (no hysteresis); ValueError unless they are integers with 1 <= keep_off <= keep <= window <= 15."""
        keep = window // 2 + 1 if keep is None and isinstance(window, (int, np.integer)) else keep
        keep_off = keep if keep_off is None else keep_off
        for name, v in (("window", window), ("keep", keep), ("keep_off", keep_off)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("temporal %s %r, expected an integer" % (name, v))
        if not 1 <= keep_off <= keep <= window <= _lib.VC_TEMPORAL_MAX_WINDOW:
            raise ValueError("temporal window %d, keep %d, keep_off %d: expected 1 <= keep_off <= keep <= window <= %d"
                             % (window, keep, keep_off, _lib.VC_TEMPORAL_MAX_WINDOW))
        return int(window), int(keep), int(keep_off)

    def temporal_filter(self, window=5, keep=None, keep_off=None, motion=None):
        """Pushes the current carve result onto a ring of the last `window` hulls on the device and replaces it by their vote: a
        voxel enters when at least `keep` of the hulls hold it (default: the majority) and, once in, stays while at least keep_off
        do (default: keep, a plain vote); the thresholds scale with the ring while it fills, so the first call returns the hull
        as it is.  Restored voxels are coloured from the colour camera as close_hull colours (contract: include/voxcarve.h).  The
        ring survives carves; temporal_reset, set_grid / set_cameras and another window start it over.  One call per carve.
        Returns the stats as a dict: window, frames, on, off, survivors_before, survivors_after, added, removed, raw_changed,
        out_changed, temporal_ms.

        motion=True or (block, apron, search) is the motion-compensated vote (vc_hull_temporal_motion): before it counts, the
        older hulls and the previous output are aligned to the current hull by the block motion field between the last hull
        and this one (hull_motion's parameters; True is 8, None, 4), and the ring keeps the aligned hulls.  The stats gain
        block, apron, search, aligned_changed and the field's blocks, listed, moved, unique, clipped, cost0_sum, cost_sum;
        fetch_temporal_motion returns the field.  A ring filled by the other kind of call starts over."""
        window, keep, keep_off = self.temporal_thresholds(window, keep, keep_off)
        from . import motion as mo
        params = mo.vote_params(motion)
        if params is not None:
            st = mo.TemporalMotionStats()
            self._check(self._L.vc_hull_temporal_motion(self._ctx, window, keep, keep_off, params[0], params[1], params[2], 0, ctypes.byref(st)),
                        "vc_hull_temporal_motion")
            self.count = int(st.survivors_after)
            self._temporal_motion = params
            out = _stats(st)
            del out["reserved"]
            return out
        st = _lib.VcTemporalStats()
        self._check(self._L.vc_hull_temporal(self._ctx, window, keep, keep_off, 0, ctypes.byref(st)), "vc_hull_temporal")
        self.count = int(st.survivors_after)
        return _stats(st)

    def fetch_temporal(self):
        """(votes, added), u8 [S] each in record order: in how many of the ring's hulls the record's voxel is, and 1 where the last
        temporal_filter created the record (fails once a carve or a pass that changes the survivors has run since)."""
        votes, added = np.empty(self.count, dtype=np.uint8), np.empty(self.count, dtype=np.uint8)
        self._check(self._L.vc_fetch_temporal(self._ctx, _ptr(votes, ctypes.c_uint8), _ptr(added, ctypes.c_uint8)), "vc_fetch_temporal")
        return votes, added

    def fetch_temporal_motion(self):
        """The field of the last temporal_filter(motion=...) as the dict of fetch_motion (no rows for the first push of a ring);
        fails when fetch_temporal fails, and after a temporal_filter without motion."""
        from . import motion
        n = ctypes.c_uint64(0)
        self._check(self._L.vc_fetch_temporal_motion(self._ctx, None, ctypes.byref(n)), "vc_fetch_temporal_motion")
        raw = np.zeros(int(n.value), dtype=motion.ROW_DTYPE)
        if n.value:
            self._check(self._L.vc_fetch_temporal_motion(self._ctx, raw.ctypes.data_as(ctypes.c_void_p), None), "vc_fetch_temporal_motion")
        return motion.rows_dict(raw, self.grid, *getattr(self, "_temporal_motion", (8, 4, 4)))

    def temporal_history(self, age):
        """The hull that temporal_filter pushed `age` calls ago (0 = the last one, always raw; with motion= the older ones as the
        calls since have aligned them) as occupancy words, uint64 [ceil(N / 64)] laid out as vc_fetch_occupancy; fails for an
        age the ring does not hold."""
        raw = np.empty((self.n_voxels + 63) // 64 if self.grid is not None else 0, dtype=np.uint64)
        self._check(self._L.vc_fetch_temporal_history(self._ctx, int(age), raw.ctypes.data_as(_lib.c_u8p)), "vc_fetch_temporal_history")
        return raw

    def temporal_reset(self):
        """Forgets the ring of hulls and the previous output: the next temporal_filter returns its hull as it is."""
        self._check(self._L.vc_temporal_reset(self._ctx), "vc_temporal_reset")

    # -- set algebra on hulls (vc_hull_keep / upload / combine / compare): a second operand for the current result -----------------
    SETOPS = {"copy": _lib.VC_SETOP_COPY, "and": _lib.VC_SETOP_AND, "or": _lib.VC_SETOP_OR, "andnot": _lib.VC_SETOP_ANDNOT,
              "xor": _lib.VC_SETOP_XOR}

    def keep_hull(self, reg=0):
        """Register `reg` (0..3) on the device becomes a copy of the current carve result, records included.  Registers survive
        carves and passes; set_grid / set_slab / set_cameras empty them."""
        self._check(self._L.vc_hull_keep(self._ctx, int(reg)), "vc_hull_keep")

    def upload_hull(self, hull, reg=0):
        """Loads a hull of the current grid into register `reg`: a bool array [n], ascending uint32 indices, or uint64 records
        (voxcarve.hullio.as_operand; only records bring colours).  The device validates it once more; a refused upload leaves
        the register as it was.  Needs a grid, not a carve result."""
        from . import hullio
        if self.grid is None:
            raise _lib.VoxcarveError("upload_hull: no grid")
        kind, data = hullio.as_operand(hull, self.n_voxels)
        if kind == "bits":
            rc = self._L.vc_hull_upload(self._ctx, int(reg), _ptr(data, ctypes.c_uint8), None, 0)
        else:
            buf = data if data.size else np.zeros(1, dtype=np.uint64)        # (n_records = 0 still names a buffer)
            rc = self._L.vc_hull_upload(self._ctx, int(reg), None, _ptr(buf, ctypes.c_uint64), int(data.size))
        self._check(rc, "vc_hull_upload")

    def release_hull(self, reg):
        """Empties register `reg` and frees its memory."""
        self._check(self._L.vc_hull_release(self._ctx, int(reg)), "vc_hull_release")

    def fetch_kept(self, reg=0):
        """Register `reg` as a dict: count, has_records, words (uint64 [ceil(n / 64)], laid out as fetch_occupancy's) and records
        (uint64 [count], or None when the register has none); fails for an empty register."""
        count, has = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._check(self._L.vc_fetch_kept(self._ctx, int(reg), None, None, ctypes.byref(count), ctypes.byref(has)), "vc_fetch_kept")
        words = np.empty((self.n_voxels + 63) // 64, dtype=np.uint64)
        records = np.empty(count.value, dtype=np.uint64) if has.value else None
        self._check(self._L.vc_fetch_kept(self._ctx, int(reg), words.ctypes.data_as(_lib.c_u8p),
                                          _ptr(records, ctypes.c_uint64) if has.value and count.value else None, None, None), "vc_fetch_kept")
        return {"count": int(count.value), "has_records": bool(has.value), "words": words, "records": records}

    def combine_hull(self, op, reg=0):
        """Replaces the current carve result A by a set operation with the hull B of register `reg`: op = "copy" (B), "and"
        (A & B: clip), "or" (union), "andnot" (A \\ B: subtract), "xor" (what differs).  Records of A that stay keep their bytes;
        a voxel that was not in A takes B's record when the register has records and is coloured from the colour camera as
        close_hull colours otherwise; "copy" from a register with records restores B's records verbatim (contract:
        include/voxcarve.h).  Returns the stats as a dict: survivors_before, other, common, survivors_after, added, removed,
        setop_ms."""
        if op not in self.SETOPS:
            raise ValueError("op %r, expected one of %s" % (op, sorted(self.SETOPS)))
        st = _lib.VcSetopStats()
        self._check(self._L.vc_hull_combine(self._ctx, self.SETOPS[op], int(reg), 0, ctypes.byref(st)), "vc_hull_combine")
        self.count = int(st.survivors_after)
        return _stats(st)

    def fetch_combined(self):
        """u8 [S] in record order: 1 where the last combine_hull brought the voxel in (fails once a carve or a pass that changes
        the survivors has run since)."""
        out = np.empty(self.count, dtype=np.uint8)
        self._check(self._L.vc_fetch_combined(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_combined")
        return out

    def compare_hull(self, reg=0, distance=False):
        """Compares the current carve result A with the hull B of register `reg` and changes nothing.  Returns a dict: a, b,
        common, only_a, only_b, diff_lo, diff_hi (the inclusive index box of the symmetric difference; UINT32_MAX and 0 when
        there is none), compare_ms; with distance=True also h2_ab, h2_ba (directed Hausdorff distances squared, um^2), arg_ab,
        arg_ba (the voxels that attain them) and q.  Derived on the host: iou = common / |A | B| and dice = 2 common / (a + b)
        (None when both hulls are empty), hausdorff_mm = sqrt(max(h2_ab, h2_ba)) / 1000 (None without distance and when
        either hull is empty)."""
        st = _lib.VcCompareStats()
        self._check(self._L.vc_hull_compare(self._ctx, int(reg), _lib.VC_COMPARE_DISTANCE if distance else 0, ctypes.byref(st)), "vc_hull_compare")
        out = _stats(st)
        if not distance:                                         # (the call left the distance fields alone)
            for name in ("h2_ab", "h2_ba", "arg_ab", "arg_ba", "q"):
                del out[name]
        union = out["common"] + out["only_a"] + out["only_b"]
        out["iou"] = out["common"] / union if union else None
        out["dice"] = 2 * out["common"] / (out["a"] + out["b"]) if union else None
        out["hausdorff_mm"] = None
        if distance:
            worst = max(out["h2_ab"], out["h2_ba"])
            if union and worst != (1 << 64) - 1:
                out["hausdorff_mm"] = float(np.sqrt(float(worst))) / 1000.0
        return out

    def save_hull(self, path):
        """Writes the current carve result (grid, bounds, records) to `path` as an .npz (voxcarve.hullio.save)."""
        from . import hullio
        hullio.save(path, self.grid, self.bounds, self.fetch_records())

    def load_hull(self, path, reg=0):
        """Loads a file of save_hull into register `reg`; ValueError when its grid or bounds are not this engine's."""
        from . import hullio
        grid, bounds, records = hullio.load(path)
        if self.grid is None or tuple(grid) != tuple(self.grid):
            raise ValueError("%s holds a hull of grid %s, the engine's is %s" % (path, grid, self.grid))
        if tuple(bounds) != tuple(self.bounds):
            raise ValueError("%s holds a hull of bounds %s, the engine's are %s" % (path, bounds, self.bounds))
        self.upload_hull(records, reg)

    def set_hull(self, hull, reg=0):
        """upload_hull(hull, reg), then combine_hull("copy", reg): the hull becomes the current result (needs a carve result to
        replace; a carve of empty masks will do).  Returns combine_hull's stats."""
        self.upload_hull(hull, reg)
        return self.combine_hull("copy", reg)

    # -- block motion between a kept hull and the current result (vc_hull_motion, vc_hull_warp, vc_paint_motion) --------------------
    def hull_motion(self, reg=0, block=8, apron=None, search=4, levels=0, refine=1):
        """Estimates where each block of `block`^3 voxels went between the hull of register `reg` (the previous frame:
        keep_hull) and the current carve result: exhaustive matching of a window of the block grown by `apron` cells per side
        (None: block // 2) over the displacements of [-search, search]^3 (contract: include/voxcarve.h).  block in {4, 8, 16},
        apron in 0..16, search in 1..8, block + 2 apron + 2 search <= 64.  Changes nothing.  Returns the stats as a dict:
        blocks, listed, moved, unique, clipped, cost0_sum, cost_sum, a, b, motion_ms.

        levels = L in 1..3 is the coarse-to-fine field (vc_hull_motion_pyramid): both hulls are halved L times, the coarsest
        level is matched as above, and every finer level chooses among the displacements within `refine` (1..search) of twice its
        parent block's vector and of twice the vectors of the parent's face neighbours, so vectors up to
        reach = search 2^L + refine (2^L - 1) voxels are found.  The dict then also holds levels, refine, reach, listed_level and
        dims_level (lists over the levels 0..3), evaluated and borrowed.  The field is fetch_motion's, warp_hull's and
        paint_motion's either way; fetch_motion_level and fetch_motion_occupancy return the coarser levels."""
        from . import motion
        block, apron, search = motion.check_params(block, apron, search)
        levels, refine = motion.check_pyramid(levels, refine, search)
        if levels == 0:
            st = motion.MotionStats()
            self._check(self._L.vc_hull_motion(self._ctx, int(reg), block, apron, search, 0, ctypes.byref(st)), "vc_hull_motion")
            self._motion = (block, apron, search)
            self._motion_pyramid = (0, refine, search)
            return _stats(st)
        st = motion.PyramidStats()
        self._check(self._L.vc_hull_motion_pyramid(self._ctx, int(reg), block, apron, search, levels, refine, 0, ctypes.byref(st)),
                    "vc_hull_motion_pyramid")
        self._motion = (block, apron, search)
        self._motion_pyramid = (levels, refine, int(st.reach))
        return motion.pyramid_stats_dict(st)

    def fetch_motion(self):
        """The field of the last hull_motion as a dict of arrays over the listed blocks, ascending block index: block u32 [L],
        ijk int64 [L, 3] (the block's position in blocks), d i8 [L, 3] (voxels, x y z), cost, cost0 u32, count_a, count_b,
        ties u16, flags u8 (bit 0: clipped by the search range); and the scalars grid, edge, apron, search.  After
        hull_motion(levels > 0) flags has bit 1 too (borrowed from a neighbour's prediction) and the dict gains the scalars
        levels, refine and reach; after a single-level call it is the dict it always was.  Fails once a carve or a pass has
        changed the hull, or the register has been written."""
        out = self.fetch_motion_level(0)
        if not out["levels"]:
            for key in ("levels", "refine", "reach"):
                del out[key]
        return out

    def fetch_motion_level(self, level):
        """The rows of level `level` (0..levels) of the last hull_motion as the dict of fetch_motion; grid is that level's (level
        0 is the field itself).  Fails when fetch_motion fails, and for a level the field does not have."""
        from . import motion
        level = int(level)
        name = "vc_fetch_motion_level" if level else "vc_fetch_motion"
        call = (lambda rows, n: self._L.vc_fetch_motion_level(self._ctx, level, rows, n)) if level else \
            (lambda rows, n: self._L.vc_fetch_motion(self._ctx, rows, n))
        n = ctypes.c_uint64(0)
        self._check(call(None, ctypes.byref(n)), name)
        raw = np.zeros(int(n.value), dtype=motion.ROW_DTYPE)
        if n.value:
            self._check(call(raw.ctypes.data_as(ctypes.c_void_p), None), name)
        levels, refine, reach = getattr(self, "_motion_pyramid", (0, 1, getattr(self, "_motion", (8, 4, 4))[2]))
        out = motion.rows_dict(raw, motion.level_grid(self.grid, level), *getattr(self, "_motion", (8, 4, 4)))
        out.update(levels=levels, refine=refine, reach=reach)
        return out

    def fetch_motion_occupancy(self, level, which):
        """uint64 [ceil(n_l / 64)]: the occupancy words of level `level` of the last hull_motion, which = 0 the current result's
        (A), 1 the register's (B); 64 cells per word in the level's linear order (iz nx_l + ix) ny_l + iy."""
        n = ctypes.c_uint64(0)
        self._check(self._L.vc_fetch_motion_occupancy(self._ctx, int(level), int(which), None, ctypes.byref(n)), "vc_fetch_motion_occupancy")
        words = np.zeros(int(n.value), dtype=np.uint64)
        if n.value:
            self._check(self._L.vc_fetch_motion_occupancy(self._ctx, int(level), int(which), words.ctypes.data_as(_lib.c_u64p), None),
                        "vc_fetch_motion_occupancy")
        return words

    def warp_hull(self, src=0, dst=1):
        """Writes to register `dst` the prediction of the current result from the hull of register `src` and the field of the
        last hull_motion(src): every listed block gathers the old hull's bits by its vector.  Returns a dict: warped, common, a,
        warp_ms and predicted_iou = common / |P | A| (None when both are empty)."""
        from . import motion
        st = motion.WarpStats()
        self._check(self._L.vc_hull_warp(self._ctx, int(src), int(dst), 0, ctypes.byref(st)), "vc_hull_warp")
        out = _stats(st)
        union = out["warped"] + out["a"] - out["common"]
        out["predicted_iou"] = out["common"] / union if union else None
        return out

    def paint_motion(self):
        """Recolours the current result in place by the field of the last hull_motion: channel = 128 + 127 d / search, x -> r,
        y -> g, z -> b (grey = at rest).  The next carve gives the camera colours again."""
        self._check(self._L.vc_paint_motion(self._ctx), "vc_paint_motion")

    # -- ray-cast images of the current result (vc_render) --------------------------------------------------------------------------
    def render(self, views, H, W, shade=None, background=(0, 0, 0)):
        """Ray-casts the current carve result (after color_visible / photo_carve / filter_components, as fetch sees it) from each
        camera.Camera of `views` (lens distortion included; self._cams are the calibrated ones) at H x W pixels -- contract:
        include/voxcarve.h.  shade: 7 u8, one per face (2a: entered while moving along +axis a, 2a + 1: along -a, 6: the
        camera sits inside the voxel; None = all 255) scaling the records' RGB; background: RGB of the misses.
        Returns a dict: rgb u8 [V, H, W, 3], depth f32 [V, H, W] (+inf on a miss), index u32 [V, H, W] (0xFFFFFFFF on a miss),
        face u8 [V, H, W] (255 on a miss) and stats (pixels, hits, cells_visited, blocks_skipped, render_ms)."""
        views = list(views)
        if not views:
            raise ValueError("render: no views")
        arr = (_lib.VcView * len(views))()
        for k, cam in enumerate(views):
            K = np.asarray(cam.K, dtype=np.float64).reshape(3, 3)
            if K[0, 1] != 0.0:
                raise ValueError("render: view %d has a skewed camera matrix (K[0,1] = %r)" % (k, float(K[0, 1])))
            arr[k].K[:] = [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])]
            arr[k].dist[:] = [float(v) for v in np.asarray(cam.dist, dtype=np.float64).reshape(5)]
            arr[k].R[:] = [float(v) for v in np.asarray(cam.R, dtype=np.float64).reshape(9)]
            arr[k].t[:] = [float(v) for v in np.asarray(cam.tvec, dtype=np.float64).reshape(3)]
        sh = None if shade is None else np.ascontiguousarray(shade, dtype=np.uint8).reshape(7)
        bg = np.ascontiguousarray(background, dtype=np.uint8).reshape(3)
        st = _lib.VcRenderStats()
        self._check(self._L.vc_render(self._ctx, len(views), ctypes.cast(arr, ctypes.c_void_p), int(H), int(W),
                                      None if sh is None else _ptr(sh, ctypes.c_uint8), _ptr(bg, ctypes.c_uint8), 0,
                                      ctypes.byref(st)), "vc_render")
        V, H, W = len(views), int(H), int(W)
        self._render_shape = (V, (H, W))
        out = {"rgb": np.empty((V, H, W, 3), dtype=np.uint8), "depth": np.empty((V, H, W), dtype=np.float32),
               "index": np.empty((V, H, W), dtype=np.uint32), "face": np.empty((V, H, W), dtype=np.uint8)}
        for k in range(V):
            self._check(self._L.vc_fetch_render(self._ctx, k, _ptr(out["index"][k], ctypes.c_uint32), _ptr(out["depth"][k], ctypes.c_float),
                                                _ptr(out["rgb"][k], ctypes.c_uint8), _ptr(out["face"][k], ctypes.c_uint8)),
                        "vc_fetch_render")
        out["stats"] = _stats(st)
        return out

    def silhouette_agreement(self, slot=0):
        """Renders the current result as each calibrated camera at mask size and compares the hit pixels with that camera's
        device mask of `slot`.  Returns one dict per camera: mask_px (mask pixels), hull_px (pixels the hull covers), both, and
        iou = both / (mask_px + hull_px - both) (1.0 when both are empty).  Mask pixels the hull leaves empty show where the
        other cameras disagree with this one (calibration error, mask noise)."""
        H, W = self.image_size
        idx = self.render(self._cams, H, W)["index"]
        out = []
        for c in range(self.n_cameras):
            hull = idx[c] != 0xFFFFFFFF
            mask = self.fetch_mask(c, slot) > 0
            m, h, b = int(mask.sum()), int(hull.sum()), int((mask & hull).sum())
            union = m + h - b
            out.append({"mask_px": m, "hull_px": h, "both": b, "iou": b / union if union else 1.0})
        return out

    def marching_cubes(self, volume=None, level=0.0, axes="reference"):
        """Triangle mesh of an ON/OFF volume on the device -> (verts float32 [V, 3], faces uint32 [F, 3]).
        volume: 3-D boolean array (what the reference hands to skimage.measure.marching_cubes, voxel_reconstruction.py:141);
        None = the occupancy of the last carve, reshaped as the reference does it (axes="reference": (nx, ny, nz) over the
        voxel order, assignment.py:144) or on its geometric axes (axes="grid": (nz, nx, ny), i.e. vertex = (iz, ix, iy))."""
        nv, nf = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if volume is None:
            nx, ny, _ = self.grid
            nzl = self.slab[1] - self.slab[0]
            dims = (nx, ny, nzl) if axes == "reference" else (nzl, nx, ny)
            bits = None
        else:
            vol = np.ascontiguousarray(volume).astype(bool)
            if vol.ndim != 3:
                raise ValueError("volume must be 3-D")
            dims = vol.shape
            packed = np.packbits(vol.reshape(-1), bitorder="little")
            bits = _ptr(packed, ctypes.c_uint8)
        self._check(self._L.vc_marching_cubes(self._ctx, bits, dims[0], dims[1], dims[2], float(level), ctypes.byref(nv), ctypes.byref(nf)),
                    "vc_marching_cubes")
        verts = np.empty((int(nv.value), 3), dtype=np.float32)
        faces = np.empty((int(nf.value), 3), dtype=np.uint32)
        self._check(self._L.vc_fetch_mesh(self._ctx, _ptr(verts, ctypes.c_float), _ptr(faces, ctypes.c_uint32)), "vc_fetch_mesh")
        return verts, faces

    def surface_mesh(self, refine_steps=8):
        """Surface mesh of the current carve result (after color_visible / photo_carve / filter_components, as fetch sees it) in
        world millimetres: the marching-cubes topology of marching_cubes(axes="grid"), each vertex moved along its grid edge by
        refine_steps bisection steps of the carve's own point test (its cameras, post-filtered masks and min_views) to where the
        silhouettes cross the edge -- contract: include/voxcarve.h.  Returns a dict: verts float64 [V, 3] (x, y, z mm), faces
        uint32 [F, 3] (outward), rgb uint8 [V, 3] (the ON voxel's record), refined bool [V] (False: the edge's ends disagree with
        the occupancy, the vertex sits at the edge midpoint) and stats (n_verts, n_faces, refined, unrefined, point_tests,
        surface_ms)."""
        st = _lib.VcSurfaceStats()
        self._check(self._L.vc_surface_mesh(self._ctx, int(refine_steps), 0, ctypes.byref(st)), "vc_surface_mesh")
        V, F = int(st.n_verts), int(st.n_faces)
        self._mesh_verts = V
        verts = np.empty((V, 3), dtype=np.float64)
        faces = np.empty((F, 3), dtype=np.uint32)
        rgb = np.empty((V, 3), dtype=np.uint8)
        refined = np.empty(V, dtype=np.uint8)
        self._check(self._L.vc_fetch_surface_mesh(self._ctx, _ptr(verts, ctypes.c_double), _ptr(faces, ctypes.c_uint32),
                                                  _ptr(rgb, ctypes.c_uint8), _ptr(refined, ctypes.c_uint8)), "vc_fetch_surface_mesh")
        return {"verts": verts, "faces": faces, "rgb": rgb, "refined": refined != 0, "stats": _stats(st)}

    # -- surface normals of the hull, smooth-shaded renders, mesh normals (vc_hull_normals, vc_shade_render, vc_surface_normals) ----
    def grid_steps_um(self):
        """(q_x, q_y, q_z): the grid steps rounded to whole micrometres, the metric of the distance and normal passes (0 on an
        axis of one cell, which those passes refuse)."""
        return tuple(int(np.rint(((self.bounds[2 * a + 1] - self.bounds[2 * a]) / float(n - 1)) * 1000.0)) if n > 1 else 0
                     for a, n in enumerate(self.grid))

    def normals_r2(self, radius_mm=None):
        """r2 in um^2 of the normals' ball: radius_r2(radius_mm), or (3 x the largest grid step in um)^2 for None."""
        if radius_mm is None:
            return (3 * max(self.grid_steps_um())) ** 2
        return self.radius_r2(radius_mm)

    def hull_normals(self, radius_mm=None):
        """Surface normals of the current carve result (contract: include/voxcarve.h): every survivor with a face neighbour that is
        not one gets minus the sum of the offsets, in um, to the survivors inside a ball of radius_mm millimetres around it
        (None: 3 x the largest grid step) -- a direction from solid to empty in world (x, y, z), integer and exact.  The result
        stays as it is.  Returns the stats as a dict: survivors, surface, zero (surface records whose sum is 0), offsets (cells
        of the ball), q, ext (the ball's reach in cells per axis), normals_ms."""
        r2 = self.normals_r2(radius_mm)
        if r2 >= 1 << 64:
            raise ValueError("radius^2 = %d um^2 does not fit 64 bits" % r2)
        st = _lib.VcNormalsStats()
        self._check(self._L.vc_hull_normals(self._ctx, int(r2), 0, ctypes.byref(st)), "vc_hull_normals")
        return _stats(st)

    def fetch_record_normals(self):
        """int16 [S, 4] in record order: (n_x, n_y, n_z, w), the normal scaled so that its largest component is +-32767; w = 1 on
        surface records (whose normal may still be 0, 0, 0), a zero row elsewhere.  Fails once anything has changed the hull."""
        out = np.empty((self.count, 4), dtype=np.int16)
        self._check(self._L.vc_fetch_record_normals(self._ctx, _ptr(out, ctypes.c_int16)), "vc_fetch_record_normals")
        return out

    def record_normals_unit(self):
        """float64 [S, 3] in record order: unit normals; rows without a normal stay zero."""
        v = self.fetch_record_normals()[:, :3].astype(np.float64)
        l = np.sqrt((v * v).sum(axis=1))
        return v / np.where(l == 0.0, 1.0, l)[:, None]

    def shade_render(self, light, ambient=64):
        """Shades the images of the last render() with the normals (needs hull_normals() and a render of the current result):
        light float64 [V, 3], per view the direction from the surface towards the light in world coordinates; ambient 0..255 is
        the brightness of a surface facing away.  Returns rgb u8 [V, H, W, 3]."""
        L = np.ascontiguousarray(light, dtype=np.float64)
        V, (H, W) = self._render_shape
        if L.shape != (V, 3):
            raise ValueError("shade_render: light of shape %r, expected %r" % (L.shape, (V, 3)))
        if not 0 <= int(ambient) <= 255:
            raise ValueError("shade_render: ambient %r not in 0..255" % (ambient,))
        self._check(self._L.vc_shade_render(self._ctx, _ptr(L, ctypes.c_double), int(ambient), 0), "vc_shade_render")
        rgb = np.empty((V, H, W, 3), dtype=np.uint8)
        for k in range(V):
            self._check(self._L.vc_fetch_shaded(self._ctx, k, _ptr(rgb[k], ctypes.c_uint8)), "vc_fetch_shaded")
        return rgb

    def normals_valid(self):
        """True while the normals of the last hull_normals() describe the current hull."""
        return self._L.vc_fetch_record_normals(self._ctx, None) == _lib.VC_OK

    def render_shaded(self, views, H, W, ambient=64, light=None, background=(0, 0, 0)):
        """render() with Lambert shading from the hull's normals instead of the six face brightnesses: runs hull_normals() when
        the normals are stale, then render(), then shade_render().  light: float64 [V, 3] (see shade_render); None = a headlight
        per view, the direction towards the camera, -R[2, :].  Returns render()'s dict with rgb shaded and rgb_flat render's own."""
        views = list(views)
        if light is None:
            light = [-np.asarray(cam.R, dtype=np.float64).reshape(3, 3)[2, :] for cam in views]
        if not self.normals_valid():
            self.hull_normals()
        out = self.render(views, H, W, background=background)
        out["rgb_flat"] = out["rgb"]
        out["rgb"] = self.shade_render(light, ambient)
        return out

    # -- free-viewpoint images: refined ray hits textured from the camera frames (vc_texture_render) ----------------------------------
    def visibility_valid(self):
        """True while the depth maps of the last color_visible() belong to the current hull."""
        if self.image_size is None:
            return False
        out = np.empty(self.image_size, dtype=np.float32)
        return self._L.vc_fetch_depth(self._ctx, 0, _ptr(out, ctypes.c_float)) == _lib.VC_OK

    def texture_render(self, slot=0, steps=8, reach_mm=None, depth_tolerance=None, best=2, sharpen=2, filter="bilinear"):
        """Textures the images of the last render() from the camera frames of `slot` (needs a current color_visible() and a
        render of the current result; contract: include/voxcarve.h).  Every hit is moved along its ray by `steps` bisection
        steps of the carve's own point test within reach_mm of the voxel face (None: the voxel diagonal), then coloured from the
        `best` cameras that see the point past color_visible's depth maps (depth_tolerance None: default_depth_tolerance()),
        weighted by the cosine between their direction and the viewing direction, squared `sharpen` times; filter "nearest" or
        "bilinear".  Nothing else changes.  Returns a dict: rgb u8 [V, H, W, 3] (the render's own where no camera sees the
        point), depth f32 [V, H, W], count u8 [V, H, W] (cameras blended), best_cam u8 [V, H, W] (255: none), refined bool
        [V, H, W] and stats (pixels, hits, refined, textured, fallback, point_tests, texture_ms)."""
        filters = {"nearest": 0, "bilinear": 1, 0: 0, 1: 1}
        if filter not in filters:
            raise ValueError("texture_render: filter %r is neither 'nearest' nor 'bilinear'" % (filter,))
        diag = self.default_depth_tolerance() if self.grid is not None else 0.0   # (no grid: the call reports it)
        reach = diag if reach_mm is None else float(reach_mm)
        tol = diag if depth_tolerance is None else float(depth_tolerance)
        st = _lib.VcTextureStats()
        self._check(self._L.vc_texture_render(self._ctx, int(slot), int(steps), reach, tol, int(best), int(sharpen), filters[filter], 0,
                                              ctypes.byref(st)), "vc_texture_render")
        V, (H, W) = self._render_shape
        out = {"rgb": np.empty((V, H, W, 3), dtype=np.uint8), "depth": np.empty((V, H, W), dtype=np.float32),
               "count": np.empty((V, H, W), dtype=np.uint8), "best_cam": np.empty((V, H, W), dtype=np.uint8)}
        refined = np.empty((V, H, W), dtype=np.uint8)
        for k in range(V):
            self._check(self._L.vc_fetch_textured(self._ctx, k, _ptr(out["rgb"][k], ctypes.c_uint8), _ptr(out["depth"][k], ctypes.c_float),
                                                  _ptr(out["count"][k], ctypes.c_uint8), _ptr(out["best_cam"][k], ctypes.c_uint8),
                                                  _ptr(refined[k], ctypes.c_uint8)), "vc_fetch_textured")
        out["refined"] = refined != 0
        out["stats"] = _stats(st)
        return out

    def render_textured(self, views, H, W, slot=0, steps=8, reach_mm=None, depth_tolerance=None, best=2, sharpen=2, filter="bilinear",
                        background=(0, 0, 0)):
        """render() + texture_render(): free-viewpoint images of the hull coloured from the camera frames.  Raises unless
        color_visible() is current (it is not run here: it would recolour the records).  Returns render()'s dict with rgb
        textured and rgb_voxels the render's own, depth refined and depth_voxels the render's own, count, best_cam, refined,
        stats (the render's) and texture_stats."""
        if not self.visibility_valid():
            raise _lib.VoxcarveError("render_textured: no depth maps of the current hull: call color_visible() first")
        out = self.render(views, H, W, background=background)
        tex = self.texture_render(slot, steps, reach_mm, depth_tolerance, best, sharpen, filter)
        out["rgb_voxels"], out["depth_voxels"] = out["rgb"], out["depth"]
        for k in ("rgb", "depth", "count", "best_cam", "refined"):
            out[k] = tex[k]
        out["texture_stats"] = tex["stats"]
        return out

    # -- lit renders: cast shadows, ambient occlusion and a floor (vc_light_render) ---------------------------------------------------
    def light_render(self, light, ambient=64, smooth=False, ao_reach=4.0, floor=None):
        """Lights the images of the last render() (needs a render of the current result; contract: include/voxcarve.h): every hit
        and every pixel that sees the floor casts a shadow ray to the light and sixteen occlusion rays through the hull.
        light: (x, y, z, w), w = 1 a point in world mm, w = 0 a direction from the surface towards the light ((x, y, z): a
        point); ambient 0..255: the brightness the occlusion rays share out, all a shadowed or averted surface gets; smooth:
        shade by the normals of hull_normals() (which must be current) instead of the cube faces; ao_reach: how far, in grid
        steps, an occlusion ray looks (0: none); floor: None, "auto" (lighting.auto_floor: the grid's largest z boundary, the
        x / y bounds grown by half their span, 250 mm cells in two greys) or a dict {z, rect: (x0, x1, y0, y1), cell_mm,
        rgb: two RGB triples}.  Nothing else changes.  Returns a dict: rgb u8 [V, H, W, 3], depth f32 [V, H, W] (the floor's
        where it shows), kind u8 [V, H, W] (0 background, 1 hull, 2 floor), shadow u8 [V, H, W] (1 in shadow, 2 turned away),
        ao u8 [V, H, W] (open rays, 0..16) and stats (pixels, hull_pixels, floor_pixels, shadowed, facing_away, rays_walked,
        cells_visited, blocks_skipped, light_ms)."""
        L = lighting.light_struct(light, ambient, smooth, ao_reach, floor, self.grid, getattr(self, "bounds", None))
        st = lighting.LightStats()
        self._check(self._L.vc_light_render(self._ctx, ctypes.byref(L), 0, ctypes.byref(st)), "vc_light_render")
        V, (H, W) = self._render_shape
        out = {"rgb": np.empty((V, H, W, 3), dtype=np.uint8), "depth": np.empty((V, H, W), dtype=np.float32),
               "kind": np.empty((V, H, W), dtype=np.uint8), "shadow": np.empty((V, H, W), dtype=np.uint8),
               "ao": np.empty((V, H, W), dtype=np.uint8)}
        for k in range(V):
            self._check(self._L.vc_fetch_lit(self._ctx, k, _ptr(out["rgb"][k], ctypes.c_uint8), _ptr(out["depth"][k], ctypes.c_float),
                                             _ptr(out["kind"][k], ctypes.c_uint8), _ptr(out["shadow"][k], ctypes.c_uint8),
                                             _ptr(out["ao"][k], ctypes.c_uint8)), "vc_fetch_lit")
        out["stats"] = _stats(st)
        return out

    def render_lit(self, views, H, W, light=None, ambient=64, smooth=False, ao_reach=4.0, floor="auto", background=(0, 0, 0)):
        """render() + light_render(): images of the hull with cast shadows, ambient occlusion and a floor.  light=None is a point
        light 1000 mm above (towards -z of) the first view's camera centre, lighting.light_above(views[0]); smooth=True runs
        hull_normals() when the normals are stale.  Returns render()'s dict with rgb lit and rgb_flat the render's own, depth
        with the floor's and depth_hull the render's own, kind, shadow, ao, stats (the render's) and light_stats."""
        views = list(views)
        if not views:
            raise ValueError("render_lit: no views")
        if light is None:
            light = lighting.light_above(views[0])
        if smooth and not self.normals_valid():
            self.hull_normals()
        out = self.render(views, H, W, background=background)
        lit = self.light_render(light, ambient, smooth, ao_reach, floor)
        out["rgb_flat"], out["depth_hull"] = out["rgb"], out["depth"]
        for k in ("rgb", "depth", "kind", "shadow", "ao"):
            out[k] = lit[k]
        out["light_stats"] = lit["stats"]
        return out

    def surface_normals(self):
        """int16 [V, 4]: per vertex of the last surface_mesh() the stored normal of the voxel its colour comes from (the ON end
        of its grid edge).  Needs hull_normals() and a mesh of the current result."""
        out = np.empty((self._mesh_verts, 4), dtype=np.int16)
        self._check(self._L.vc_surface_normals(self._ctx, _ptr(out, ctypes.c_int16)), "vc_surface_normals")
        return out

    # -- the hull split into K figures on the floor plane (vc_hull_clusters, vc_paint_clusters) ------------------------------------
    def cluster_hull(self, k, max_iters=32, min_column=1, init_mm=None, hist_iz=None):
        """Splits the current carve result into k figures by K-means over its columns on the floor plane (world "up" is -z;
        contract: include/voxcarve.h): every column (ix, iy) weighs the survivors above it, columns with fewer than min_column
        weigh nothing (specks).  init_mm: k world (x, y) positions in mm to start from (the previous frame's centres: label k then
        stays the same figure); None seeds farthest-first.  hist_iz = (lo, hi): the inclusive band of layers the colour signatures
        (fetch_cluster_histograms) are taken from; None is every layer.  Integers only and exact; the result stays as it is.
        Returns the stats as a dict: survivors, columns, weight, iterations, converged, q, clusters_ms, k and centres_mm (float64
        [k, 2], world mm)."""
        init = None
        if init_mm is not None:
            c = np.asarray(init_mm, dtype=np.float64)
            if c.shape != (int(k), 2) or not np.isfinite(c).all():
                raise ValueError("cluster_hull: init_mm of shape %r, expected %r finite values" % (c.shape, (int(k), 2)))
            init = np.ascontiguousarray(np.rint((c - np.array([self.bounds[0], self.bounds[2]])) * 1000.0).astype(np.int64))
        lo, hi = (0, self.grid[2] - 1) if hist_iz is None else (int(hist_iz[0]), int(hist_iz[1]))
        if lo < 0 or hi < 0:
            raise ValueError("cluster_hull: hist_iz %r is negative" % (hist_iz,))
        st = _lib.VcClusterStats()
        self._check(self._L.vc_hull_clusters(self._ctx, int(k), int(max_iters), int(min_column), lo, hi,
                                             None if init is None else _ptr(init, ctypes.c_int64), 0, ctypes.byref(st)),
                    "vc_hull_clusters")
        self._cl_k = int(k)
        return _stats(st, converged=bool(st.converged), k=int(k), centres_mm=self.fetch_clusters()["centre_mm"])

    def clusters_valid(self):
        """True while the clustering of the last cluster_hull() describes the current hull."""
        return self._L.vc_fetch_cluster_labels(self._ctx, None) == _lib.VC_OK

    def fetch_cluster_labels(self):
        """u8 [S] in record order: the figure each survivor belongs to.  Fails once anything has changed the hull."""
        out = np.empty(self.count, dtype=np.uint8)
        self._check(self._L.vc_fetch_cluster_labels(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_cluster_labels")
        return out

    def fetch_clusters(self):
        """The figures of the last cluster_hull: dict of numpy arrays centre_um int64 [K, 2] (from the grid's (x_min, y_min)
        corner), centre_mm float64 [K, 2] (world), voxels u64 [K], weight u64 [K], columns u32 [K], lo / hi u32 [K, 3] (inclusive
        box in (ix, iy, iz); lo = 0xffffffff > hi = 0 for a figure without a voxel)."""
        K = self._cl_k
        raw = (_lib.VcCluster * max(K, 1))()
        self._check(self._L.vc_fetch_clusters(self._ctx, raw), "vc_fetch_clusters")
        um = np.array([[int(v) for v in raw[k].centre_um] for k in range(K)], dtype=np.int64).reshape(K, 2)
        mm = np.array([self.bounds[0], self.bounds[2]]) + um.astype(np.float64) / 1000.0
        return {"centre_um": um, "centre_mm": mm, "voxels": np.array([raw[k].voxels for k in range(K)], dtype=np.uint64),
                "weight": np.array([raw[k].weight for k in range(K)], dtype=np.uint64),
                "columns": np.array([raw[k].columns for k in range(K)], dtype=np.uint32),
                "lo": np.array([list(raw[k].lo) for k in range(K)], dtype=np.uint32).reshape(K, 3),
                "hi": np.array([list(raw[k].hi) for k in range(K)], dtype=np.uint32).reshape(K, 3)}

    def fetch_cluster_histograms(self):
        """u32 [K, 512]: per figure the histogram of its seen records' colours in the band of cluster_hull's hist_iz, bin
        (r >> 5) << 6 | (g >> 5) << 3 | (b >> 5), with the colours the records had at that call."""
        out = np.empty((self._cl_k, 512), dtype=np.uint32)
        self._check(self._L.vc_fetch_cluster_histograms(self._ctx, _ptr(out, ctypes.c_uint32)), "vc_fetch_cluster_histograms")
        return out

    def fetch_floor_map(self):
        """u32 [nx, ny]: the survivors above each floor position."""
        nx, ny, _ = self.grid
        out = np.empty((nx, ny), dtype=np.uint32)
        self._check(self._L.vc_fetch_floor_map(self._ctx, _ptr(out, ctypes.c_uint32)), "vc_fetch_floor_map")
        return out

    def fetch_floor_labels(self):
        """u8 [nx, ny]: the figure of each floor position, 255 where no voxel stands."""
        nx, ny, _ = self.grid
        out = np.empty((nx, ny), dtype=np.uint8)
        self._check(self._L.vc_fetch_floor_labels(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_floor_labels")
        return out

    def paint_clusters(self, palette=None):
        """Recolours the current result in place: every survivor takes its figure's colour, palette u8 [K, 3] RGB (None: the
        first K of voxcarve.clusters.PALETTE).  fetch() / fetch_records(), render and mesh then show the split; the next carve
        gives the camera colours again."""
        from .clusters import PALETTE
        K = self._cl_k
        pal = np.ascontiguousarray(PALETTE[:K] if palette is None else palette, dtype=np.uint8)
        if pal.shape != (K, 3):
            raise ValueError("paint_clusters: palette of shape %r, expected %r" % (pal.shape, (K, 3)))
        if K == 0:
            pal = np.zeros((1, 3), dtype=np.uint8)               # (the call reports the missing clustering)
        self._check(self._L.vc_paint_clusters(self._ctx, _ptr(pal, ctypes.c_uint8)), "vc_paint_clusters")

    # -- geodesic distances through the hull, extremities, regions, paths (vc_hull_geodesic, vc_paint_geodesic) ------------------
    def hull_geodesic(self, seeds="floor", layers=1, extrema=0, connectivity=26, paths=False):
        """Measures every survivor's distance to the seed set along paths inside the current carve result, in whole micrometres
        (contract: include/voxcarve.h), and picks `extrema` extremities by repeated farthest-point selection: each becomes a
        source of its own, so that fetch_geodesic_labels() cuts the hull into the regions nearest to the seed set (0) and to
        extremity k (k).  seeds: "floor" (the survivors of the `layers` highest iz layers that hold any: world "up" is -z), "top"
        (the lowest iz layers) or an array of linear voxel indices, each a survivor.  paths=True also keeps the path of every
        extremity back to the nearest earlier source (stick_figure).  The result stays as it is.  Returns the stats as a dict:
        survivors, seeds, reached, unreached, max_d, tile_visits, tiles, edge_um, q, extremities, rounds, launches,
        geodesic_ms."""
        lst, n = None, 0
        if isinstance(seeds, str):
            if seeds not in ("floor", "top"):
                raise ValueError("hull_geodesic: seeds %r, expected \"floor\", \"top\" or an array of voxel indices" % (seeds,))
            mode = _lib.VC_GEO_SEEDS_IZ_MAX if seeds == "floor" else _lib.VC_GEO_SEEDS_IZ_MIN
        else:
            v = np.asarray(seeds).reshape(-1)
            if v.size and (not np.issubdtype(v.dtype, np.integer) or int(v.min()) < 0 or int(v.max()) > 0xffffffff):
                raise ValueError("hull_geodesic: seeds must be voxel indices in 0 .. 2^32 - 1")
            lst, n, mode = np.ascontiguousarray(v, dtype=np.uint32), int(v.size), _lib.VC_GEO_SEEDS_LIST
        if int(layers) < 0 or int(extrema) < 0:
            raise ValueError("hull_geodesic: layers %r, extrema %r" % (layers, extrema))
        st = _lib.VcGeodesicStats()
        self._check(self._L.vc_hull_geodesic(self._ctx, int(connectivity), mode, _ptr(lst, ctypes.c_uint32) if n else None, n, int(layers),
                                             int(extrema), _lib.VC_GEO_PATHS if paths else 0, ctypes.byref(st)), "vc_hull_geodesic")
        self._geo_k = int(st.extremities)
        return _stats(st)

    def geodesic_valid(self):
        """True while the outputs of the last hull_geodesic() describe the current hull."""
        return self._L.vc_fetch_geodesic(self._ctx, None) == _lib.VC_OK

    def fetch_geodesic(self):
        """u64 [S] in record order: the distance to the nearest source in um, 2^64 - 1 where unreached."""
        out = np.empty(self.count, dtype=np.uint64)
        self._check(self._L.vc_fetch_geodesic(self._ctx, _ptr(out, ctypes.c_uint64)), "vc_fetch_geodesic")
        return out

    def fetch_geodesic_mm(self):
        """float64 [S]: the same in mm, inf where unreached."""
        d = self.fetch_geodesic()
        return np.where(d == np.uint64(0xffffffffffffffff), np.inf, d.astype(np.float64) / 1000.0)

    def fetch_geodesic_labels(self):
        """u8 [S]: the region of every survivor -- 0 nearest to the seed set, k nearest to extremity k, 255 unreached."""
        out = np.empty(self.count, dtype=np.uint8)
        self._check(self._L.vc_fetch_geodesic_labels(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_geodesic_labels")
        return out

    def fetch_extrema(self):
        """The extremities of the last hull_geodesic, in the order they were picked: dict of numpy arrays label u32 [E] (1 .. E),
        voxel u32, record u32, d u64 (um, when picked), d_mm float64, index u32 [E, 3] (ix, iy, iz), world_mm float64 [E, 3]."""
        E = self._geo_k
        raw = (_lib.VcExtremum * max(E, 1))()
        self._check(self._L.vc_fetch_extrema(self._ctx, raw), "vc_fetch_extrema")
        index = np.array([[raw[k].ix, raw[k].iy, raw[k].iz] for k in range(E)], dtype=np.uint32).reshape(E, 3)
        d = np.array([raw[k].d for k in range(E)], dtype=np.uint64)
        return {"label": np.array([raw[k].label for k in range(E)], dtype=np.uint32),
                "voxel": np.array([raw[k].voxel for k in range(E)], dtype=np.uint32),
                "record": np.array([raw[k].record for k in range(E)], dtype=np.uint32), "d": d, "d_mm": d.astype(np.float64) / 1000.0,
                "index": index, "world_mm": self.voxel_world_mm(index[:, 0], index[:, 1], index[:, 2])}

    def voxel_world_mm(self, ix, iy, iz):
        """float64 [n, 3]: the world position in mm of the voxels (ix, iy, iz)."""
        xs, ys, zs = self.axes()
        return np.stack([xs[np.asarray(ix, dtype=np.int64)], ys[np.asarray(iy, dtype=np.int64)], zs[np.asarray(iz, dtype=np.int64)]],
                        axis=1).reshape(-1, 3)

    def _path(self, call, what, arg):
        n = ctypes.c_uint32(0)
        cap = sum(self.grid)
        for _ in range(2):
            out = np.empty(max(cap, 1), dtype=np.uint32)
            rc = call(self._ctx, int(arg), _ptr(out, ctypes.c_uint32), cap, ctypes.byref(n))
            if rc == _lib.VC_OK or n.value <= cap:
                break
            cap = n.value                                         # (the call said how long the path is)
        self._check(rc, what)
        return out[:n.value].copy()

    def geodesic_path(self, voxel):
        """u32 [n]: the linear indices of the shortest path from `voxel` (a reached survivor) to a voxel with d = 0, `voxel` first,
        through the keys as the last hull_geodesic left them."""
        return self._path(self._L.vc_geodesic_path, "vc_geodesic_path", voxel)

    def stick_figure(self):
        """The paths of all extremities of the last hull_geodesic(paths=True), each back to the nearest source that existed when
        it was picked (the seed set or an earlier extremity): a list of float64 [n, 3] arrays in world mm, extremity first."""
        nx, ny, _ = self.grid
        out = []
        for k in range(1, self._geo_k + 1):
            i = self._path(self._L.vc_fetch_extremum_path, "vc_fetch_extremum_path", k).astype(np.int64)
            out.append(self.voxel_world_mm((i // ny) % nx, i % ny, i // (nx * ny)))
        if not out:
            self._check(self._L.vc_fetch_extrema(self._ctx, None), "vc_fetch_extrema")       # (reports a missing pass)
        return out

    def fetch_extremum_path(self, k):
        """u32 [n]: the linear indices of stick_figure()'s path k (1-based)."""
        return self._path(self._L.vc_fetch_extremum_path, "vc_fetch_extremum_path", k)

    def paint_geodesic(self, mode="labels", palette=None):
        """Recolours the current result in place: mode "labels" gives every survivor its region's colour, palette u8 [>= regions, 3]
        RGB (None: voxcarve.geodesic.PALETTE); mode "distance" a grey ramp 255 d div max_d.  Unreached voxels take
        voxcarve.geodesic.UNREACHED_RGB.  fetch() / fetch_records(), render and mesh then show it; the next carve gives the
        camera colours again."""
        from .geodesic import MAX_K, PALETTE
        if mode not in ("labels", "distance"):
            raise ValueError("paint_geodesic: mode %r, expected \"labels\" or \"distance\"" % (mode,))
        pal = np.zeros((MAX_K + 1, 3), dtype=np.uint8)
        src = np.asarray(PALETTE if palette is None else palette, dtype=np.uint8)
        if src.ndim != 2 or src.shape[1] != 3 or src.shape[0] > MAX_K + 1 or (mode == "labels" and src.shape[0] < self._geo_k + 1):
            raise ValueError("paint_geodesic: palette of shape %r, expected [%d .. %d, 3]" % (src.shape, self._geo_k + 1, MAX_K + 1))
        pal[:src.shape[0]] = src
        self._check(self._L.vc_paint_geodesic(self._ctx, _lib.VC_GEO_PAINT_LABELS if mode == "labels" else _lib.VC_GEO_PAINT_DISTANCE,
                                              _ptr(pal, ctypes.c_uint8)), "vc_paint_geodesic")

    # -- the hull's figures measured per group of records (vc_hull_measure) --------------------------------------------------------
    def component_ranks(self):
        """(u32 [S], components): per record of the current hull the rank of its connected component, size descending then label
        ascending -- the host labels of measure_hull(labels="components").  Needs a filter_components that is current and
        removed nothing from its input (its labels are in its input's record order): otherwise ValueError."""
        try:
            lab = self.fetch_component_labels()
            comp = self.fetch_components()
        except _lib.VoxcarveError as exc:
            raise ValueError('measure_hull(labels="components"): no components of the current hull (%s): run filter_components '
                             "once more on its own output" % exc) from exc
        if lab.size != self.count or not comp["kept"].all():
            raise ValueError('measure_hull(labels="components"): the last filter_components removed voxels, its labels describe '
                             "its input: run filter_components once more on its own output")
        order = np.lexsort((comp["label"], -comp["size"].astype(np.int64)))
        rank = np.empty(order.size, dtype=np.uint32)
        rank[order] = np.arange(order.size, dtype=np.uint32)
        return rank[np.searchsorted(comp["label"], lab)], int(order.size)

    def measure_hull(self, labels="all", groups=None, profile=False):
        """Reduces the records of the current carve result to a few integers per group (contract: include/voxcarve.h): voxels,
        surface voxels, seen voxels, first and second moments of (ix, iy, iz), exposed faces per direction, colour sums, box --
        and with profile=True {n, sum ix, sum iy} per group and layer.  labels: "all" (one group), "clusters" (the figures of a
        current cluster_hull), "geodesic" (the regions of a current hull_geodesic; unreached voxels belong to no group),
        "components" (the connected components of a current filter_components that removed nothing, ranked by size descending
        then label ascending) or an integer array [S] in record order with `groups` = G (0xffffffff: no group).  Integers only
        and exact; the result stays as it is.  voxcarve.measure.describe() turns the integers into mm.  Returns the stats as a
        dict: survivors, groups, measured, unlabelled, measure_ms."""
        src, lab, G = _lib.VC_MEASURE_ALL, None, 0
        if isinstance(labels, str):
            if labels == "clusters":
                src = _lib.VC_MEASURE_CLUSTERS
            elif labels == "geodesic":
                src = _lib.VC_MEASURE_GEODESIC
            elif labels == "components":
                lab, G = self.component_ranks()
                src = _lib.VC_MEASURE_HOST
                if G == 0:                                       # (an empty hull has no component: one empty group)
                    G = 1
            elif labels != "all":
                raise ValueError('measure_hull: labels %r, expected "all", "clusters", "geodesic", "components" or an integer array' % (labels,))
        else:
            v = np.asarray(labels).reshape(-1)
            if v.size and (not np.issubdtype(v.dtype, np.integer) or int(v.min()) < 0 or int(v.max()) > 0xffffffff):
                raise ValueError("measure_hull: labels must be integers in 0 .. 2^32 - 1")
            if v.size != self.count:
                raise ValueError("measure_hull: %d labels for %d records" % (v.size, self.count))
            if groups is None:
                raise ValueError("measure_hull: an array of labels needs groups=G")
            if not 0 <= int(groups) <= 0xffffffff:
                raise ValueError("measure_hull: groups %r" % (groups,))
            src, lab, G = _lib.VC_MEASURE_HOST, v, int(groups)
        if lab is not None:
            lab = np.ascontiguousarray(lab, dtype=np.uint32)
            if lab.size == 0:
                lab = np.zeros(1, dtype=np.uint32)               # (a pointer the call can tell from NULL)
        st = _lib.VcMeasureStats()
        self._check(self._L.vc_hull_measure(self._ctx, src, None if lab is None else _ptr(lab, ctypes.c_uint32), G,
                                            _lib.VC_MEASURE_PROFILE if profile else 0, ctypes.byref(st)), "vc_hull_measure")
        self._ms_g = int(st.groups)
        return _stats(st)

    def measure_valid(self):
        """True while the measurements of the last measure_hull() describe the current hull."""
        return self._L.vc_fetch_measure(self._ctx, None) == _lib.VC_OK

    def fetch_measure(self):
        """The groups of the last measure_hull: dict of numpy arrays voxels, surface, seen u64 [G], s1 u64 [G, 3] (sum ix, iy,
        iz), s2 u64 [G, 6] (sum ix^2, iy^2, iz^2, ix iy, ix iz, iy iz), faces u64 [G, 6] (-x, +x, -y, +y, -z, +z), rgb u64 [G, 3]
        (over the seen records), lo / hi u32 [G, 3] (inclusive box in (ix, iy, iz); lo = 0xffffffff > hi = 0 for an empty group)."""
        G = self._ms_g
        raw = np.zeros((max(G, 1), 24), dtype=np.uint64)
        self._check(self._L.vc_fetch_measure(self._ctx, raw.ctypes.data_as(ctypes.POINTER(_lib.VcMeasure))), "vc_fetch_measure")
        raw = raw[:G]
        box = np.ascontiguousarray(raw[:, 21:24]).view(np.uint32).reshape(G, 6)
        return {"voxels": raw[:, 0].copy(), "surface": raw[:, 1].copy(), "seen": raw[:, 2].copy(), "s1": raw[:, 3:6].copy(),
                "s2": raw[:, 6:12].copy(), "faces": raw[:, 12:18].copy(), "rgb": raw[:, 18:21].copy(), "lo": box[:, :3].copy(),
                "hi": box[:, 3:].copy()}

    def fetch_measure_profile(self):
        """u64 [G, nz, 3]: per group and layer iz {n, sum ix, sum iy} of the last measure_hull(profile=True) -- the cross-section
        and, divided by n, its centre line by height."""
        G = self._ms_g
        out = np.zeros((max(G, 1), self.grid[2], 3), dtype=np.uint64)
        self._check(self._L.vc_fetch_measure_profile(self._ctx, _ptr(out, ctypes.c_uint64)), "vc_fetch_measure_profile")
        return out[:G]

    # -- the hull's shell: what a viewer of opaque cubes can see (vc_hull_shell) ---------------------------------------------------
    def hull_shell(self, level=0):
        """Lists the cells of the current carve result that have an exposed face, in cell order, with their exposed faces
        (contract: include/voxcarve.h): at level 0 the surface voxels with their records' colours, at level L in 1..6 the cells
        of a grid 2^L times coarser with the rounded mean colour of the surface voxels inside them that the colour camera sees.
        Everything a ray can hit is in the level-0 shell; the hull itself stays as it is.  Returns the stats as a dict:
        survivors, cells_on, shell, faces [6] (-x, +x, -y, +y, -z, +z), level, cube_scale (2^level: the edge of the cube to draw
        per cell, in voxels), dims (the coarse grid), shell_ms."""
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or level < 0:
            raise ValueError("hull_shell: level %r, expected an integer in 0..%d" % (level, _lib.VC_SHELL_MAX_LEVEL))
        st = _lib.VcShellStats()
        self._check(self._L.vc_hull_shell(self._ctx, int(level), 0, ctypes.byref(st)), "vc_hull_shell")
        self._shell_t = int(st.shell)
        return _stats(st, faces=[int(v) for v in st.faces], dims=[int(v) for v in st.dims])     # (these two have been lists)

    def shell_valid(self):
        """True while the list of the last hull_shell() describes the current hull."""
        return self._L.vc_fetch_shell(self._ctx, None, None) == _lib.VC_OK

    def fetch_shell(self):
        """(records u64 [T], faces u8 [T]) of the last hull_shell: per shell cell {u32 cell index, r, g, b, seen} and the byte of
        its exposed faces (bit k: -x, +x, -y, +y, -z, +z), ascending by cell."""
        T = self._shell_t
        rec = np.zeros(max(T, 1), dtype=np.uint64)
        faces = np.zeros(max(T, 1), dtype=np.uint8)
        self._check(self._L.vc_fetch_shell(self._ctx, _ptr(rec, ctypes.c_uint64), _ptr(faces, ctypes.c_uint8)), "vc_fetch_shell")
        return rec[:T], faces[:T]

    def fetch_shell_viewer(self, scaling_factor=SCALING_FACTOR):
        """(positions float32 [T, 3], colors float32 [T, 3]) of the last hull_shell, made on the device: at level 0 exactly
        viewer_positions(voxel_keys(...)) and viewer_colors(...) of the shell's voxels; above it the centre of each coarse cell
        (draw its cube cube_scale times as large)."""
        T = self._shell_t
        pos = np.zeros((max(T, 1), 3), dtype=np.float32)
        col = np.zeros((max(T, 1), 3), dtype=np.float32)
        self._check(self._L.vc_fetch_shell_viewer(self._ctx, float(scaling_factor), _ptr(pos, ctypes.c_float), _ptr(col, ctypes.c_float)),
                    "vc_fetch_shell_viewer")
        return pos[:T], col[:T]

    # -- the hull thinned to a curve skeleton (vc_hull_thin) -----------------------------------------------------------------------
    def thin_hull(self, mode="curve", anchors=None, max_passes=_lib.VC_THIN_DEFAULT_PASSES):
        """Thins the current carve result to a centred, one-voxel-wide skeleton with the hull's components, tunnels and cavities
        (contract: include/voxcarve.h).  mode "curve" keeps end points, so limbs stay lines; "point" shrinks every component to
        a topological kernel.  anchors: None, "extrema" (the voxels at distance 0 of a current hull_geodesic: its seeds and its
        extremities) or linear indices of survivors, which are never removed.  The hull itself stays as it is.  Returns the
        stats as a dict: survivors, anchors, kept, removed, passes, steps, launches, stable, isolated, endpoints, junctions,
        thin_ms."""
        if mode not in ("curve", "point"):
            raise ValueError('thin_hull: mode %r, expected "curve" or "point"' % (mode,))
        if not 1 <= int(max_passes) <= _lib.VC_THIN_MAX_PASSES:
            raise ValueError("thin_hull: max_passes %r not in 1 .. %d" % (max_passes, _lib.VC_THIN_MAX_PASSES))
        src, lst = _lib.VC_THIN_ANCHORS_NONE, None
        if isinstance(anchors, str):
            if anchors != "extrema":
                raise ValueError('thin_hull: anchors %r, expected None, "extrema" or linear indices' % (anchors,))
            src = _lib.VC_THIN_ANCHORS_EXTREMA
        elif anchors is not None:
            v = np.asarray(anchors).reshape(-1)
            if v.size and (not np.issubdtype(v.dtype, np.integer) or int(v.min()) < 0 or int(v.max()) > 0xffffffff):
                raise ValueError("thin_hull: anchors must be linear indices in 0 .. 2^32 - 1")
            src, lst = _lib.VC_THIN_ANCHORS_LIST, np.ascontiguousarray(v, dtype=np.uint32)
        st = _lib.VcThinStats()
        self._check(self._L.vc_hull_thin(self._ctx, _lib.VC_THIN_CURVE if mode == "curve" else _lib.VC_THIN_POINT, src,
                                         None if lst is None or lst.size == 0 else _ptr(lst, ctypes.c_uint32),
                                         0 if lst is None else lst.size, int(max_passes), 0, ctypes.byref(st)), "vc_hull_thin")
        self._thin = (int(st.survivors), int(st.kept))
        return _stats(st)

    def thin_valid(self):
        """True while the skeleton of the last thin_hull() describes the current hull."""
        return self._L.vc_fetch_thin(self._ctx, None) == _lib.VC_OK

    def fetch_thin(self):
        """u16 [S]: per record 0 when the last thin_hull kept its voxel, else 1 + 6 (pass - 1) + d of the direction step that
        removed it -- the order in which the hull was peeled."""
        S = self._thin[0]
        out = np.zeros(max(S, 1), dtype=np.uint16)
        self._check(self._L.vc_fetch_thin(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))), "vc_fetch_thin")
        return out[:S]

    def fetch_skeleton(self):
        """The kept voxels of the last thin_hull, ascending by voxel: dict of voxel u32 [K], record u32 [K], degree u8 [K] (the
        kept voxels among the 26 neighbours) and index i64 [K, 3] = (ix, iy, iz)."""
        K = self._thin[1]
        raw = np.zeros((max(K, 1), 3), dtype=np.uint32)
        self._check(self._L.vc_fetch_skeleton(self._ctx, raw.ctypes.data_as(ctypes.POINTER(_lib.VcSkeletonVoxel))), "vc_fetch_skeleton")
        raw = raw[:K]
        nx, ny, _ = self.grid
        i = raw[:, 0].astype(np.int64)
        return {"voxel": raw[:, 0].copy(), "record": raw[:, 1].copy(), "degree": (raw[:, 2] & 0xff).astype(np.uint8),
                "index": np.stack([(i // ny) % nx, i % ny, i // (nx * ny)], axis=1)}

    def fetch_thin_table(self):
        """u8 [2^23]: bit c (byte c >> 3, bit c & 7) says whether a voxel whose 26 neighbours have the code c is simple -- the
        table thin_hull looks up with option thin_table = 1, built on the device at first use."""
        out = np.zeros(_lib.VC_THIN_TABLE_BYTES, dtype=np.uint8)
        self._check(self._L.vc_fetch_thin_table(self._ctx, _ptr(out, ctypes.c_uint8)), "vc_fetch_thin_table")
        return out

    def set_option(self, name, value):
        """Launch-geometry tuning knobs (never change results); see vc_set_option."""
        self._check(self._L.vc_set_option(self._ctx, name.encode(), int(value)), "vc_set_option")

    def debug_counters(self):
        out = np.zeros(8, dtype=np.uint64)
        self._check(self._L.vc_debug_counters(self._ctx, _ptr(out, ctypes.c_uint64)), "vc_debug_counters")
        return {"bricks_listed": int(out[0]), "bricks_live": int(out[1]), "bricks_full": int(out[2]), "bricks": int(out[3]),
                "columns_listed": int(out[4]), "words_undecided": int(out[5]),
                # the expansion launched last read the colour camera's compact table (option emit_lut16) | such a table exists
                "emit_lut16": int(out[6]), "lut16_table": int(out[7])}

    def synchronize(self):
        self._check(self._L.vc_synchronize(self._ctx), "vc_synchronize")

    def timing(self, reset=False):
        t = _lib.VcTiming()
        self._check(self._L.vc_timing(self._ctx, ctypes.byref(t)), "vc_timing")
        if reset:
            self._check(self._L.vc_timing_reset(self._ctx), "vc_timing_reset")
        out = {name: getattr(t, name) for name, _ in _lib.VcTiming._fields_ if name not in ("kernel_ms_sum", "kernel_launches", "work")}
        out["kernels"] = {k: {"ms_sum": float(t.kernel_ms_sum[i]), "launches": int(t.kernel_launches[i])}
                          for i, k in enumerate(_lib.KERNEL_KINDS) if t.kernel_launches[i]}
        out["work"] = {k: int(t.work[i]) for i, k in enumerate(_lib.WORK_KINDS)}
        return out

    # -- multi-GPU -------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        L = _lib.load()
        buf = (ctypes.c_uint8 * _lib.VC_UNIQUE_ID_BYTES)()
        _lib.check(L.vc_comm_unique_id(buf), None, "vc_comm_unique_id")
        return bytes(buf)

    def comm_init(self, n_ranks, rank, uid):
        import os
        import sys
        if "torch" in sys.modules and os.environ.get("VOXCARVE_ALLOW_TORCH") != "1":
            # Measured on the GPU box: a torch wheel bundles its own libhsa-runtime64 / librccl; once it is
            # loaded, RCCL resolves HSA from that uninitialised copy and ncclCommInitRank fails with
            # "no ROCm-capable device is detected".  Exchange the unique id without a framework
            # (slabs.file_rendezvous) or set VOXCARVE_ALLOW_TORCH=1 if your torch uses the system ROCm.
            raise _lib.VoxcarveError("comm_init in a process that imported torch: its bundled ROCm runtime breaks RCCL "
                                     "(see voxcarve.slabs.file_rendezvous); set VOXCARVE_ALLOW_TORCH=1 to try anyway")
        buf = (ctypes.c_uint8 * _lib.VC_UNIQUE_ID_BYTES).from_buffer_copy(uid)
        self._check(self._L.vc_comm_init(self._ctx, n_ranks, rank, buf), "vc_comm_init")
        self.n_ranks, self.rank = n_ranks, rank

    def comm_destroy(self):
        self._check(self._L.vc_comm_destroy(self._ctx), "vc_comm_destroy")

    def allgather(self):
        """RCCL all-gather of all ranks' survivor records; returns (counts per rank, total)."""
        counts = np.zeros(self.n_ranks, dtype=np.uint64)
        total = ctypes.c_uint64(0)
        self._check(self._L.vc_allgather(self._ctx, _ptr(counts, ctypes.c_uint64), ctypes.byref(total)),
                    "vc_allgather")
        self.gathered_total = int(total.value)
        return counts, self.gathered_total

    def comm_max(self, value=0.0):
        """Max of `value` over all ranks through RCCL; with the default it is a barrier."""
        v = ctypes.c_double(float(value))
        self._check(self._L.vc_comm_allreduce_max(self._ctx, ctypes.byref(v)), "vc_comm_allreduce_max")
        return v.value

    def fetch_gathered(self):
        rec = np.empty(self.gathered_total, dtype=np.uint64)
        self._check(self._L.vc_fetch_gathered(self._ctx, _ptr(rec, ctypes.c_uint64)), "vc_fetch_gathered")
        return rec

    # -- compact exchange form (host-side transports, tests) ---------------------------
    def pack_entries(self):
        """The last carve's non-zero occupancy words as u64 [M,2] = {bits, global index of bit 0}, ascending."""
        m = ctypes.c_uint64(0)
        self._check(self._L.vc_pack_entries(self._ctx, ctypes.byref(m)), "vc_pack_entries")
        ent = np.empty((int(m.value), 2), dtype=np.uint64)
        self._check(self._L.vc_fetch_entries(self._ctx, _ptr(ent, ctypes.c_uint64)), "vc_fetch_entries")
        return ent

    def expand_entries(self, entries):
        """All ranks' entries in rank order -> ordered records of the whole grid on this device (read them with
        fetch_gathered()), coloured like this engine's last carve.  Returns the survivor count."""
        ent = np.ascontiguousarray(entries, dtype=np.uint64).reshape(-1, 2)
        total = ctypes.c_uint64(0)
        self._check(self._L.vc_expand_entries(self._ctx, _ptr(ent, ctypes.c_uint64), ent.shape[0],
                                              ctypes.byref(total)), "vc_expand_entries")
        self.gathered_total = int(total.value)
        return self.gathered_total


# -- record / viewer helpers (host arithmetic of assignment.py:127-133) ----------------
def unpack_records(rec):
    """u64 records -> (idx u32, rgb u8 [S,3], seen bool)."""
    rec = np.ascontiguousarray(rec, dtype=np.uint64)
    b = rec.view(np.uint8).reshape(-1, 8)
    return rec.astype(np.uint32), b[:, 4:7].copy(), (b[:, 7] & 1).astype(bool)


def voxel_keys(idx, grid, axes):
    """tuple(map(int, voxel)) of voxel_reconstruction.py:84: truncated coordinates int64 [S,3]."""
    nx, ny, _ = grid
    xs, ys, zs = axes
    idx = np.asarray(idx, dtype=np.int64)
    iy = idx % ny
    t = idx // ny
    return np.stack([np.trunc(xs[t % nx]), np.trunc(ys[iy]), np.trunc(zs[t // nx])], axis=1).astype(np.int64)


def viewer_positions(keys, scaling_factor=SCALING_FACTOR):
    """assignment.py:127-130: x = vx/64, y = -(vz/64), z = vy/64 -> float32 [S,3] (as mesh.py:82 casts)."""
    k = np.asarray(keys, dtype=np.int64)
    pos = np.stack([k[:, 0] / scaling_factor, -(k[:, 2] / scaling_factor), k[:, 1] / scaling_factor], axis=1)
    return pos.astype(np.float32)


def viewer_colors(rgb):
    """assignment.py:133: BGR[::-1] / 255.0 -> float32 [S,3] (as mesh.py:88 casts)."""
    return (np.asarray(rgb, dtype=np.uint8) / 255.0).astype(np.float32)
