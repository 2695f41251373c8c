"""Cost of the ray caster (vc_render) over a carve result: (a) 1024^3 with the 4 real cameras and the committed MOG
masks, 8 orbit views at 1920x1080, with and without block skipping (option render_blocks); (b) 128^3 (the reference's size),
the 4 calibrated views with their distortion at 644x486.  Per case: render_ms (HIP events around the whole call, median of the
repetitions), ms per view, Mrays/s, cells looked at and blocks skipped per ray, hit fraction.  The block map's build time is
taken as the render of one 1x1 view whose ray misses the grid, with skipping minus without (only the map build differs).  At
1024^3 also one photo_carve round of the same hull for comparison.  --out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _render(eng, views, H, W, reps, blocks=1):
    eng.set_option("render_blocks", blocks)
    ms, st = [], None
    for _ in range(reps + 1):
        r = eng.render(views, H, W)
        st = r["stats"]
        ms.append(st["render_ms"])
    eng.set_option("render_blocks", 1)
    med = float(np.median(ms[1:]))
    px = st["pixels"]
    return {"views": len(views), "image": [H, W], "blocks": blocks, "render_ms": med, "ms_per_view": med / len(views),
            "mrays_per_s": px / med / 1e3, "cells_per_ray": st["cells_visited"] / px, "skips_per_ray": st["blocks_skipped"] / px,
            "hit_fraction": st["hits"] / px}


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import camera
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n in (1024, 128):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            for c, f in enumerate(frames):
                eng.upload_frame(c, f)
            S = eng.carve()
            case = {"grid": n, "survivors": S}
            eye = np.array([10256.0, 0.0, -768.0])                 # outside the grid, looking away from it: the ray misses
            one = [camera.look_at(eye, eye + (1000.0, 0.0, 0.0), 1.0, 1, 1)]
            on = _render(eng, one, 1, 1, 9, 1)["render_ms"]
            off = _render(eng, one, 1, 1, 9, 0)["render_ms"]
            case["map_ms"] = on - off
            if n == 1024:
                orbit = camera.orbit(8, 4500.0, 25.0, 1500.0, 1080, 1920)
                case["orbit_blocks"] = _render(eng, orbit, 1080, 1920, 5, 1)
                case["orbit_voxels"] = _render(eng, orbit, 1080, 1920, 3, 0)
                st = eng.photo_carve(max_rounds=1)
                case["photo_one_round_ms"] = st["photo_ms"]
            else:
                case["calibrated_blocks"] = _render(eng, cams, H0, W0, 9, 1)
                case["calibrated_voxels"] = _render(eng, cams, H0, W0, 9, 0)
            res[str(n)] = case
            print(json.dumps(case), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
