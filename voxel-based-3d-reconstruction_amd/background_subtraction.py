"""The reference's ``extract_foreground_mask`` (background_subtraction.py:129-208) and its MOG and MOG2 background models
(``train_MOG_background_model``, :49-92; ``train_MOG2_background_model``, :90-127) with their data-parallel stages on the GPU.

SURVEY 8(f)-2, the step BEFORE the carve path.  Same names, parameters and defaults as the reference's functions.  What runs where:

  BGR -> HSV (:155)                      GPU   CarveEngine.bgr_to_hsv          (OpenCV's 8-bit fixed-point conversion)
  bg_model.apply (:158)                  GPU   BackgroundSubtractorMOG.apply   (the model assignment.py:79 trains; per pixel mixture
                                               of Gaussians, state in HBM)
                                         GPU   BackgroundSubtractorMOG2.apply  (Zivkovic's adaptive mixture, cv2's MOG2; shadows
                                               marked shadowValue, 127 by default, state in HBM)
                                         CPU   whatever other model the caller hands in (a cv2 KNN object works as before)
  3x3 open / close before the contours   GPU   CarveEngine.mask_morphology(.., 3, ..)
  contours: fill the figures, re-open
  their large holes (:171-193)           GPU   CarveEngine.fill_figures (contour_stage="device"): components, their containment
                                               tree and per-cell areas in place of border following (csrc/vc_contour.h)
                                         CPU   fill_figures, the default: cv2.findContours / fillPoly / drawContours
  2x2 open / close after them (:195-203) GPU   CarveEngine.mask_morphology(.., 2, ..)
  final threshold (:206)                 host  one comparison

With a device model and contour_stage="device" no stage needs cv2 (each GPU call here copies its image down and back);
CarveEngine.foreground_to_slot runs the whole function for every camera into a carve slot, with nothing coming back
(assignment.DeviceVideoSource).
The cv2 stage needs cv2 (as the reference does), and so does decoding the training video; without it those calls fail by name.
Parity of the GPU stages with cv2 is unpinned: the contour stage is held to a literal restatement of the published border
following, fillPoly and drawContours (tests/contour_literal.py), the others to oracle/foreground_np.py, oracle/mog_np.py and
tests/mog2_np.py."""
import sys

import numpy as np

from ._lib import VoxcarveError

_engine = None


def _default_engine():
    global _engine
    if _engine is None:
        from .engine import CarveEngine
        _engine = CarveEngine(0)
    return _engine


class BackgroundSubtractorMOG:
    """cv2.bgsegm.createBackgroundSubtractorMOG(history, nmixtures, backgroundRatio, noiseSigma) with the model on the device
    (background_subtraction.py:75-76).  ``apply(image, fgmask=None, learningRate=-1)`` as cv2's: uint8 [H,W,3] in, uint8 [H,W]
    {0, 255} out; -1 = 1 / min(frames seen, history), 0 = the model is only read (the reference's inference, :158)."""

    def __init__(self, history=200, nmixtures=5, backgroundRatio=0.7, noiseSigma=0, engine=None):
        self._eng = engine if engine is not None else _default_engine()
        self._model = self._eng.mog_create(history, nmixtures, backgroundRatio, noiseSigma)

    def apply(self, image, fgmask=None, learningRate=-1):
        out = self._eng.mog_apply(self._model, image, learningRate)
        if fgmask is not None:
            fgmask[...] = out
            return fgmask
        return out

    def state(self):
        return self._eng.mog_state(self._model)

    def close(self):
        if self._model is not None:
            self._eng.mog_destroy(self._model)
            self._model = None

    def __del__(self):
        if sys.is_finalizing():                  # as CarveEngine.__del__: no HIP call from a finalising interpreter; the process's
            return                               # exit takes the model with the context
        try:
            self.close()
        except Exception:
            pass


class BackgroundSubtractorMOG2:
    """cv2.createBackgroundSubtractorMOG2(history, varThreshold, detectShadows) with the model on the device
    (background_subtraction.py:110-111).  The keyword-only arguments are the values cv2 fixes at construction (settable there
    through setters before the first frame); nmixtures may be 1..8 here.  ``apply(image, fgmask=None, learningRate=-1)`` as
    cv2's: uint8 [H,W,3] in, uint8 [H,W] {0, shadowValue, 255} out; -1 = 1 / min(2 frames seen, history).  Unlike MOG, learning
    rate 0 still writes the model (its weights are renormalised)."""

    def __init__(self, history=500, varThreshold=16, detectShadows=True, *, nmixtures=5, backgroundRatio=0.9, varThresholdGen=9,
                 varInit=15, varMin=4, varMax=75, complexityReductionThreshold=0.05, shadowValue=127, shadowThreshold=0.5,
                 engine=None):
        self._eng = engine if engine is not None else _default_engine()
        self._model = None
        self._model = self._eng.mog2_create(history, varThreshold, detectShadows, nmixtures, backgroundRatio, varThresholdGen, varInit,
                                            varMin, varMax, complexityReductionThreshold, shadowValue, shadowThreshold)
        f = lambda v: float(np.float32(v))                     # cv2 keeps these as float and hands them back as double
        self._params = dict(history=int(history) if history > 0 else 500, varThreshold=f(varThreshold if varThreshold > 0 else 16),
                            detectShadows=bool(detectShadows), nmixtures=int(nmixtures), backgroundRatio=f(backgroundRatio),
                            varThresholdGen=f(varThresholdGen), varInit=f(varInit), varMin=f(varMin), varMax=f(varMax),
                            complexityReductionThreshold=f(complexityReductionThreshold), shadowValue=int(shadowValue),
                            shadowThreshold=f(shadowThreshold))

    def apply(self, image, fgmask=None, learningRate=-1):
        out = self._eng.mog2_apply(self._model, image, learningRate)
        if fgmask is not None:
            fgmask[...] = out
            return fgmask
        return out

    def getHistory(self): return self._params["history"]
    def getNMixtures(self): return self._params["nmixtures"]
    def getVarThreshold(self): return self._params["varThreshold"]
    def getDetectShadows(self): return self._params["detectShadows"]
    def getShadowValue(self): return self._params["shadowValue"]
    def getShadowThreshold(self): return self._params["shadowThreshold"]
    def getBackgroundRatio(self): return self._params["backgroundRatio"]
    def getVarThresholdGen(self): return self._params["varThresholdGen"]
    def getVarInit(self): return self._params["varInit"]
    def getVarMin(self): return self._params["varMin"]
    def getVarMax(self): return self._params["varMax"]
    def getComplexityReductionThreshold(self): return self._params["complexityReductionThreshold"]

    def state(self):
        """(state float32 [5 nmixtures, H W], nmodes uint8 [H W], (H, W), frames seen): CarveEngine.mog2_state."""
        return self._eng.mog2_state(self._model)

    def close(self):
        if self._model is not None:
            self._eng.mog2_destroy(self._model)
            self._model = None

    def __del__(self):
        if sys.is_finalizing():                  # as CarveEngine.__del__: no HIP call from a finalising interpreter; the process's
            return                               # exit takes the model with the context
        try:
            self.close()
        except Exception:
            pass


def _video_frames(path, who="train_MOG_background_model"):
    try:
        import cv2
    except ImportError as exc:
        raise VoxcarveError("%s: decoding %s runs on cv2.VideoCapture, which is not importable here (%s); "
                            "pass the frames themselves (frames=...)" % (who, path, exc))
    cap = cv2.VideoCapture(path)
    if not cap.isOpened():
        return None

    def gen():
        while True:
            ok, frame = cap.read()
            if not ok:
                return
            yield frame
    return gen()


def train_MOG_background_model(bg_video_input_path="data/cam", bg_video_input_filename="background.avi", use_hsv=True,
                               history=200, n_mixtures=5, bg_ratio=0.7, noise_sigma=0, learning_rate=-1, engine=None, frames=None):
    """A MOG model trained on a background video; reference background_subtraction.py:49-92, same parameters (None if the video
    cannot be opened, as there).  ``frames``: an iterable of BGR frames instead of the video file (no cv2 needed then)."""
    import os
    if frames is None:
        frames = _video_frames(os.path.join(bg_video_input_path, bg_video_input_filename))
        if frames is None:
            return None
    eng = engine if engine is not None else _default_engine()
    model = BackgroundSubtractorMOG(history=history, nmixtures=n_mixtures, backgroundRatio=bg_ratio, noiseSigma=noise_sigma, engine=eng)
    for frame in frames:
        if use_hsv:
            frame = eng.bgr_to_hsv(frame)
        model.apply(frame, None, learning_rate)
    return model


def train_MOG2_background_model(bg_video_input_path="data/cam", bg_video_input_filename="background.avi", use_hsv=True,
                                history=500, var_threshold=16, detect_shadows=True, learning_rate=-1, engine=None, frames=None):
    """A MOG2 model trained on a background video; reference background_subtraction.py:90-127, same parameters (None if the video
    cannot be opened, as there).  ``frames``: an iterable of BGR frames instead of the video file (no cv2 needed then)."""
    import os
    if frames is None:
        frames = _video_frames(os.path.join(bg_video_input_path, bg_video_input_filename), "train_MOG2_background_model")
        if frames is None:
            return None
    eng = engine if engine is not None else _default_engine()
    model = BackgroundSubtractorMOG2(history=history, varThreshold=var_threshold, detectShadows=detect_shadows, engine=eng)
    for frame in frames:
        if use_hsv:
            frame = eng.bgr_to_hsv(frame)
        model.apply(frame, None, learning_rate)
    return model


def fill_figures(mask, figure_threshold, figure_inner_threshold):
    """The contour stage (:171-193) with cv2: every contour of the RETR_TREE hierarchy whose area reaches ``figure_threshold``
    is drawn filled; each of its direct children whose oriented area reaches ``figure_inner_threshold`` is cleared again and
    its outline kept."""
    try:
        import cv2
    except ImportError as exc:
        raise VoxcarveError("extract_foreground_mask: the contour stage (findContours / fillPoly, background_subtraction.py:171-193) "
                            "runs on cv2, which is not importable here (%s)" % exc)
    contours, hierarchy = cv2.findContours(mask, cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE)
    out = np.zeros(mask.shape, dtype=np.uint8)
    for k, outer in enumerate(contours):
        if cv2.contourArea(outer) < figure_threshold:
            continue
        cv2.drawContours(out, [outer], -1, 255)
        cv2.fillPoly(out, [outer], 255)
        child = hierarchy[0][k][2]                            # first child; siblings follow through field 0
        while child != -1:
            hole = contours[child]
            if cv2.contourArea(hole, True) >= figure_inner_threshold:
                cv2.fillPoly(out, [hole], 0)
                cv2.drawContours(out, [hole], -1, 255)
            child = hierarchy[0][child][0]
    return out


def fill_figures_device(mask, figure_threshold, figure_inner_threshold, engine=None):
    """fill_figures on the GPU (CarveEngine.fill_figures): the same stage without cv2."""
    eng = engine if engine is not None else _default_engine()
    return eng.fill_figures(mask, figure_threshold, figure_inner_threshold)


def extract_foreground_mask(image, bg_model, learning_rate=0, figure_threshold=5000, figure_inner_threshold=115,
                            apply_opening_pre=False, apply_closing_pre=False, apply_opening_post=False,
                            apply_closing_post=False, engine=None, contour_stage=None):
    """Foreground mask (uint8 {0, 255} [H, W]) of a BGR image; reference background_subtraction.py:129-208, same parameters.
    ``engine``: the CarveEngine whose device does the work (default: one on device 0); ``contour_stage``: None = ``fill_figures``
    (cv2), "device" = ``fill_figures_device``, or a callable standing in for it (tests)."""
    eng = engine if engine is not None else _default_engine()
    if contour_stage == "device":
        contour_stage = lambda m, ft, fit: fill_figures_device(m, ft, fit, eng)
    if isinstance(bg_model, (BackgroundSubtractorMOG, BackgroundSubtractorMOG2)) and bg_model._eng is eng:
        # the model lives on this device: colour conversion, apply and pre-filter without leaving it
        model_mask = eng.foreground_front(bg_model._model, image, learning_rate, apply_opening_pre, apply_closing_pre)
    else:
        hsv = eng.bgr_to_hsv(image)
        model_mask = np.ascontiguousarray(bg_model.apply(hsv, None, learning_rate), dtype=np.uint8)
        if apply_opening_pre or apply_closing_pre:
            model_mask = eng.mask_morphology(model_mask, 3, apply_opening_pre, apply_closing_pre)
    figures = (contour_stage or fill_figures)(model_mask, figure_threshold, figure_inner_threshold)
    if apply_opening_post or apply_closing_post:
        figures = eng.mask_morphology(figures, 2, apply_opening_post, apply_closing_post)
    return np.where(figures > 0, 255, 0).astype(np.uint8)
