"""The texturing pass's restatement (tests/texture_np.py) on the CPU: the vectorised form against the literal one on every output,
the invariants of the bisection, a calibrated camera's own view (the pixels it colours alone are its frame's pixels), and what
the pass is worth against an analytic frame of a view no camera has; the library's exports."""
import functools
import math

import numpy as np
import pytest

import fixtures_util as fx
import render_np as rn
import surface_np as sn
import texture_np as tn
import visible_np as vn
from oracle import carve_np
from voxcarve import camera, synthetic

RIG_RADII = (250.0, 200.0, 300.0)
RIG_HW = (240, 320)
CONFIGS = [  # steps, best (0: every camera), sharpen, filter -- every value of every option, not their product
    (0, 1, 0, 0), (1, 2, 4, 1), (24, 0, 0, 1), (24, 1, 4, 0), (0, 0, 4, 1), (1, 1, 0, 1), (24, 2, 0, 0), (0, 2, 0, 1)]


def hull(grid, bounds, cams, masks, frames, m):
    """The carve, vc_color_visible and what the texturing pass reads of them, restated: dict occ, idx, rgb, zmaps, masks, tol."""
    H, W = masks[0].shape
    oc = fx.oracle_cams(cams)
    r = carve_np.carve(*grid, oc, masks, frames, bounds=bounds, min_views=m)
    idx = r["idx"].astype(np.int64)
    tol = vn.default_tolerance(grid, bounds)
    zmaps, _, rgb = vn.color_visible(idx, r["bgr"][:, ::-1], grid, bounds, oc, frames, H, W, tol)
    occ = np.zeros(grid[0] * grid[1] * grid[2], dtype=bool)
    occ[idx] = True
    return {"occ": occ, "idx": idx, "rgb": rgb, "zmaps": zmaps, "masks": np.stack([mk > 0 for mk in masks]), "tol": tol,
            "grid": grid, "bounds": bounds, "cams": oc, "frames": frames, "m": m}


def rendered(h, views, H, W):
    vp = [rn.view_params(v) for v in views]
    r = rn.render(h["occ"], h["idx"], h["rgb"], h["grid"], h["bounds"], vp, H, W)
    return vp, r["index"] != rn.MISS, r["depth"], r["rgb"]


def textured(h, vp, H, W, hit, depth, rgb, k, form=tn.texture_view, **kw):
    return form(vp[k], H, W, hit[k], depth[k], rgb[k], h["cams"], h["masks"], h["m"], h["zmaps"], h["frames"], **kw)


def _literal_equals_vectorised(h, views, H, W, per_view=160, seed=0):
    vp, hit, depth, rgb = rendered(h, views, H, W)
    C = len(h["cams"])
    rng = np.random.default_rng(seed)
    checked = refined = blended = 0
    for steps, best, sharpen, filt in CONFIGS:
        kw = dict(steps=steps, reach=h["tol"], tol=h["tol"], best=best or C, sharpen=sharpen, filt=filt)
        for k in range(len(views)):
            vec = textured(h, vp, H, W, hit, depth, rgb, k, **kw)
            hp, mp = np.nonzero(hit[k])[0], np.nonzero(~hit[k])[0]
            px = np.concatenate([rng.choice(hp, min(per_view, hp.size), replace=False), mp[:8]]).astype(np.int64)
            lit = textured(h, vp, H, W, hit, depth, rgb, k, form=tn.texture_literal, pixels=px, **kw)
            for key in ("rgb", "count", "best_cam", "refined"):
                assert np.array_equal(vec[key][px], lit[key]), (key, steps, best, sharpen, filt, k)
            assert np.array_equal(vec["depth"][px].view(np.uint32), lit["depth"].view(np.uint32)), (steps, best, sharpen, filt, k)
            st = vec["stats"]
            assert st["hits"] == int(hit[k].sum()) and st["textured"] + st["fallback"] == st["hits"]
            assert st["refined"] == int(vec["refined"].sum()) and st["textured"] == int((vec["count"] > 0).sum())
            checked += px.size
            refined += int(lit["refined"].sum())
            blended += int((lit["count"] > 1).sum())
    return checked, refined, blended


def test_vectorised_equals_literal_golden_cameras():
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    h = hull((32, 32, 32), carve_np.DEFAULT_BOUNDS, cams, masks, frames, 4)
    views = camera.orbit(2, 4500.0, 25.0, 90.0, 61, 83)
    checked, refined, blended = _literal_equals_vectorised(h, views, 61, 83)
    assert checked > 1000 and refined > 100 and blended > 100
    # a calibrated camera (lens distortion) at its own size, a strided sample of its pixels
    vp, hit, depth, rgb = rendered(h, cams[:1], *masks[0].shape)
    px = np.nonzero(hit[0])[0][::97]
    kw = dict(steps=8, reach=h["tol"], tol=h["tol"], best=2, sharpen=2, filt=1)
    vec = textured(h, vp, *masks[0].shape, hit, depth, rgb, 0, **kw)
    lit = textured(h, vp, *masks[0].shape, hit, depth, rgb, 0, form=tn.texture_literal, pixels=px, **kw)
    assert px.size > 50
    for key in ("rgb", "count", "best_cam", "refined"):
        assert np.array_equal(vec[key][px], lit[key]), key
    assert np.array_equal(vec["depth"][px].view(np.uint32), lit["depth"].view(np.uint32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_vectorised_equals_literal_random_scenes(seed):
    cams, masks, frames = fx.random_scene(seed, C=3, H=37, W=53)
    h = hull((20, 18, 22), carve_np.DEFAULT_BOUNDS, cams, masks, frames, 2)
    views = camera.orbit(2, 4000.0, 30.0, 40.0, 24, 32)
    checked, _, _ = _literal_equals_vectorised(h, views, 24, 32, per_view=60, seed=seed)
    assert checked > 300


def _rig():
    cams = camera.orbit(6, 2500.0, 20.0, 500.0, *RIG_HW) + camera.orbit(2, 2500.0, 70.0, 500.0, *RIG_HW)
    masks, frames = synthetic.textured_scene(cams, *RIG_HW, shape="ellipsoid", radii=RIG_RADII)
    c = synthetic.VOLUME_CENTRE
    bounds = (c[0] - 400.0, c[0] + 400.0, c[1] - 400.0, c[1] + 400.0, c[2] - 400.0, c[2] + 400.0)
    return cams, masks, frames, bounds


@functools.lru_cache(maxsize=None)
def rig_hull(n):
    cams, masks, frames, bounds = _rig()
    return cams, hull((n, n, n), bounds, cams, masks, frames, 8)


def novel_view():
    c = np.asarray(synthetic.VOLUME_CENTRE)
    a, e = math.radians(30.0), math.radians(35.0)
    eye = c + 2500.0 * np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), -math.sin(e)])
    return camera.look_at(eye, c, 500.0, *RIG_HW)


def test_bisection_invariants():
    cams, h = rig_hull(32)
    H, W = RIG_HW
    vp, hit, depth, rgb = rendered(h, [novel_view()], H, W)
    inside = lambda o, d, t: sn.count_views(tn._points(o, d, t), h["cams"], h["masks"]) >= h["m"]
    for steps, L in ((8, h["tol"]), (24, h["tol"]), (3, 5000.0)):
        r = textured(h, vp, H, W, hit, depth, rgb, 0, steps=steps, reach=L, tol=h["tol"], with_interval=True)
        ref = r["refined"][r["px"]] != 0
        assert ref.sum() > 100
        o, d, lo, hi = r["o"], r["d"][ref], r["lo"][ref], r["hi"][ref]
        assert inside(o, d, hi).all() and not inside(o, d, lo).any()
        free = ~r["clamped"][ref]
        if L > 3000.0:
            assert (~free).any()                       # the eye is 2500 mm away: a reach beyond it clamps lo to 0
            assert np.all(r["lo0"][ref][~free] == 0.0)
        # t0 -+ L rounds once (an ulp of the far end at the most), every midpoint once more (half an ulp each)
        width, far = hi[free] - lo[free], r["t0"][ref][free] + L
        assert np.all(np.abs(width - L * 2.0 ** -steps) <= (steps + 2) * np.spacing(far))
        assert np.array_equal(r["depth"][r["px"]][ref], ((lo + hi) * 0.5).astype(np.float32))


@pytest.mark.parametrize("n", [32, 64])
def test_own_view_returns_the_cameras_own_pixels(n):
    """From a calibrated camera's own pose, with one camera per pixel, no sharpening and the nearest pixel, every pixel that
    camera colours is its frame's pixel bit for bit, and those are at least 95 % of the hits (measured with this restatement:
    see DESIGN.md section 8 item 22)."""
    cams, h = rig_hull(n)
    H, W = RIG_HW
    own = (0, 6)
    vp, hit, depth, rgb = rendered(h, [cams[k] for k in own], H, W)
    for k, c in enumerate(own):
        r = textured(h, vp, H, W, hit, depth, rgb, k, steps=0, reach=h["tol"], tol=h["tol"], best=1, sharpen=0, filt=0)
        mine = hit[k] & (r["best_cam"] == c)
        frame_rgb = np.asarray(h["frames"][c]).reshape(-1, 3)[:, ::-1]
        assert np.array_equal(r["rgb"][mine], frame_rgb[mine])
        share = mine.sum() / hit[k].sum()
        print("own view: grid %d camera %d: %.2f %% of %d hits" % (n, c, 100.0 * share, hit[k].sum()))
        assert share >= 0.95


def _error(img, want, where):
    return float(np.abs(img.reshape(-1, 3)[where].astype(np.int64) - want.reshape(-1, 3)[where].astype(np.int64)).mean())


@pytest.mark.parametrize("n", [32, 64])
def test_texturing_with_refinement_is_worth_it(n):
    """Against the analytic frame of a view half-way between two cameras, over the hit pixels inside the true mask: the mean
    absolute channel error of the textured image (8 steps, best 2, sharpen 2, bilinear) is at most 0.7 x that of the voxel
    colours.  steps = 0 is printed, not asserted: without the refinement the parallax of a voxel-sized depth error eats the gain."""
    cams, h = rig_hull(n)
    H, W = RIG_HW
    view = novel_view()
    true_mask, true_frame = synthetic.textured_scene([view], H, W, shape="ellipsoid", radii=RIG_RADII)
    want = true_frame[0][..., ::-1]
    vp, hit, depth, rgb = rendered(h, [view], H, W)
    where = hit[0] & (true_mask[0].reshape(-1) > 0)
    assert where.sum() > 5000
    kw = dict(reach=h["tol"], tol=h["tol"], best=2, sharpen=2, filt=1)
    e_vox = _error(rgb[0], want, where)
    e_0 = _error(textured(h, vp, H, W, hit, depth, rgb, 0, steps=0, **kw)["rgb"], want, where)
    e_8 = _error(textured(h, vp, H, W, hit, depth, rgb, 0, steps=8, **kw)["rgb"], want, where)
    print("worth: grid %d: voxel colours %.2f, textured 0 steps %.2f, textured 8 steps %.2f (ratio %.2f)" % (n, e_vox, e_0, e_8, e_8 / e_vox))
    assert e_8 <= 0.7 * e_vox


def test_library_exports_the_pass(built):
    from voxcarve import _lib
    header = open(fx.ROOT + "/include/voxcarve.h").read()
    for name, nargs in (("vc_texture_render", 10), ("vc_fetch_textured", 7)):
        assert "int %s(vc_ctx *ctx" % name in header and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    import voxcarve
    for name in ("texture_render", "render_textured", "visibility_valid"):
        assert hasattr(voxcarve.CarveEngine, name)
