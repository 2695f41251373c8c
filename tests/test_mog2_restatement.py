"""The MOG2 restatement (tests/mog2_np.py) against itself -- the vectorised form against the literal per-pixel one, mask and every
state bit -- and against what the model must do; plus the exports and signature of the MOG2 pieces of the package.  No GPU.
Parity with cv2 itself: unpinned (cv2 is not here)."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import mog2_np

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxel-based-3d-reconstruction_amd")


def _frames(rng, shape, n):
    """A background of flat and textured regions, sensor noise, a second mode that comes and goes, a moving inverted square,
    and a darkened (shadow-like) band in some frames."""
    H, W = shape
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    bg[: H // 2] = (bg[: H // 2] // 8) + 130
    alt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = []
    for t in range(n):
        f = (alt if t % 5 == 4 else bg).astype(np.int64) + rng.integers(-6, 7, (H, W, 3))
        if t % 3 == 2:
            f[: max(H // 3, 1)] = (f[: max(H // 3, 1)] * 7) // 10
        if t >= n // 2 and H > 4 and W > 4:
            y, x = (3 * t) % (H - 3), (5 * t) % (W - 3)
            f[y:y + 3, x:x + 3] = 255 - f[y:y + 3, x:x + 3]
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


SCHEDULE = [-1] * 10 + [0.05] * 3 + [0, 0] + [1.0] + [-1] * 3 + [0, 0.3, 0.002, 0]


def _run_pair(kw, shape, schedule, seed, resize_at=None):
    rng = np.random.default_rng(seed)
    vec, lit = mog2_np.MOG2(**kw), mog2_np.MOG2Literal(**kw)
    frames = _frames(rng, shape, len(schedule))
    for t, (f, lr) in enumerate(zip(frames, schedule)):
        if resize_at is not None and t == resize_at:
            f = rng.integers(0, 256, (shape[0] + 1, shape[1], 3), dtype=np.uint8)
        a, b = vec.apply(f, lr), lit.apply(f, lr)
        assert np.array_equal(a, b), (kw, t, lr, int((a != b).sum()))
        assert np.array_equal(vec.state.view(np.uint32), lit.state.view(np.uint32)), (kw, t, lr)
        assert np.array_equal(vec.nmodes, lit.nmodes), (kw, t, lr)
        assert vec.nframes == lit.nframes and (vec.nmodes <= vec.K).all()
    return vec


@pytest.mark.parametrize("K", [1, 3, 5, 8])
@pytest.mark.parametrize("shadows", [True, False])
def test_vectorised_equals_literal(K, shadows):
    kw = dict(nmixtures=K, detectShadows=shadows)
    if K == 3:
        kw.update(history=7, varThreshold=30, shadowThreshold=0.3, shadowValue=90)
    if K == 8:
        kw.update(varThreshold=650, shadowThreshold=0.7, shadowValue=200, complexityReductionThreshold=0.2)
    _run_pair(kw, (7, 11), SCHEDULE, seed=K * 2 + shadows)
    _run_pair(kw, (5, 6), SCHEDULE[:12], seed=K, resize_at=6)


def test_rare_branches_occur_and_agree():
    """Pruning (weight below -prune: n shrinks inside the mode loop), replacing the weakest mode when all K are in use, and the
    renormalisation that learning rate 0 still performs -- each happens on these sequences, and both forms agree through it."""
    kw = dict(nmixtures=2, complexityReductionThreshold=0.6, varThresholdGen=4, varThreshold=25)
    vec = _run_pair(kw, (9, 13), SCHEDULE, seed=3)
    assert vec.stats.get("pruned", 0) > 0 and vec.stats.get("replaced", 0) > 0, vec.stats
    # learning rate 0 writes the model: weights renormalised (and never a new mode)
    rng = np.random.default_rng(8)
    m = mog2_np.MOG2(nmixtures=4)
    frames = _frames(rng, (16, 16), 12)
    for f in frames[:10]:
        m.apply(f, -1)
    before, modes = m.state.copy(), m.nmodes.copy()
    m.apply(frames[10], 0)
    w_before, w_after = before.reshape(4, 5, -1)[:, 0], m.state.reshape(4, 5, -1)[:, 0]
    assert not np.array_equal(w_before.view(np.uint32), w_after.view(np.uint32))
    assert (m.nmodes <= modes).all()


def test_behaviour():
    rng = np.random.default_rng(1)
    H, W = 12, 16
    bg = rng.integers(120, 256, (H, W, 3), dtype=np.uint8)                       # bright: every channel >= 120
    noisy = lambda: np.clip(bg.astype(np.int64) + rng.integers(-2, 3, bg.shape), 0, 255).astype(np.uint8)
    for shadows in (True, False):
        m = mog2_np.MOG2(history=50, detectShadows=shadows)
        for _ in range(40):
            m.apply(noisy(), -1)
        assert (m.apply(noisy(), 0) == 0).all()                                  # the trained background is background
        obj = noisy()
        obj[3:9, 4:12] = 255 - obj[3:9, 4:12]                                     # something never seen
        assert (m.apply(obj, 0)[3:9, 4:12] == 255).all()
        dark = (bg.astype(np.float64) * 0.7).astype(np.uint8)                     # the background in shadow
        got = m.apply(dark, 0)
        assert (got == (127 if shadows else 255)).all(), np.unique(got)
        assert (m.nmodes <= m.K).all()
    m = mog2_np.MOG2(history=50, shadowValue=60, shadowThreshold=0.6)
    for _ in range(40):
        m.apply(noisy(), -1)
    assert (m.apply((bg.astype(np.float64) * 0.7).astype(np.uint8), 0) == 60).all()
    assert (m.apply((bg.astype(np.float64) * 0.5).astype(np.uint8), 0) == 255).all()   # darker than tau allows


def test_package_exports_mog2(built):
    """The built library exports the MOG2 entry points, and the drop-in trainer has the reference's parameters and defaults
    (background_subtraction.py:90-91)."""
    lib = ctypes.CDLL(os.path.join(PKG, "libvoxcarve.so"))
    for name in ("vc_mog2_create", "vc_mog2_apply", "vc_mog2_state", "vc_mog2_destroy"):
        assert hasattr(lib, name), name
    from voxcarve import background_subtraction as bs
    sig = inspect.signature(bs.train_MOG2_background_model)
    want = [("bg_video_input_path", "data/cam"), ("bg_video_input_filename", "background.avi"), ("use_hsv", True), ("history", 500),
            ("var_threshold", 16), ("detect_shadows", True), ("learning_rate", -1)]
    got = [(p.name, p.default) for p in sig.parameters.values()][:len(want)]
    assert got == want
    assert {"engine", "frames"} <= set(sig.parameters)
    sig2 = inspect.signature(bs.BackgroundSubtractorMOG2)
    assert [(p.name, p.default) for p in sig2.parameters.values()][:3] == [("history", 500), ("varThreshold", 16), ("detectShadows", True)]
