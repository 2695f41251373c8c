"""Cost of the texturing pass (vc_texture_render) with the 4 real cameras and the committed MOG masks at 128^3 and
1024^3: the 4 calibrated cameras at their own 486 x 644, and 4 orbit views at 1080p.  Per case texture_ms (HIP events around the
whole call, median of the repetitions) at 8 steps / best 2 / sharpen 2 / bilinear and at 0 steps, hits, refined, textured,
point_tests, and the two yardsticks on the same hull: render_ms of vc_render for the same views and visible_ms of one
vc_color_visible pass; the ratios texture / render and texture / visible.  --reps N (default 11), --quick (3 repetitions),
--out FILE keeps the numbers as JSON.  The texture calls fetch their images to the host as CarveEngine.texture_render does;
the times are the device's.  Needs an MI355X."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _texture(eng, steps, reps):
    ms, st = [], None
    for _ in range(reps + 1):                                      # the first call allocates: left out
        st = eng.texture_render(steps=steps)["stats"]
        ms.append(st["texture_ms"])
    return {"steps": steps, "texture_ms": float(np.median(ms[1:])), "min_ms": float(np.min(ms[1:])), "hits": st["hits"],
            "refined": st["refined"], "textured": st["textured"], "fallback": st["fallback"], "point_tests": st["point_tests"],
            "tests_per_hit": st["point_tests"] / st["hits"] if st["hits"] else 0.0}


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import camera
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 11
    if "--quick" in sys.argv:
        reps = 3
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    views = {"cameras_486x644": (cams, H0, W0), "orbit_1080p": (camera.orbit(4, 4500.0, 25.0, 1500.0, 1080, 1920), 1080, 1920)}
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n in (128, 1024):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            for c, f in enumerate(frames):
                eng.upload_frame(c, f)
            case = {"grid": n, "cameras": 4, "survivors": eng.carve()}
            vis = []
            for _ in range(reps + 1):
                eng.color_visible()
                vis.append(eng.timing()["visible_ms"])
            case["visible_ms"] = float(np.median(vis[1:]))
            for name, (vw, H, W) in views.items():
                rms = [eng.render(vw, H, W)["stats"]["render_ms"] for _ in range(reps + 1)]
                v = {"views": len(vw), "H": H, "W": W, "render_ms": float(np.median(rms[1:]))}
                v["steps8"] = _texture(eng, 8, reps)
                v["steps0"] = _texture(eng, 0, reps)
                v["texture_over_render"] = v["steps8"]["texture_ms"] / v["render_ms"]
                v["texture_over_visible"] = v["steps8"]["texture_ms"] / case["visible_ms"]
                case[name] = v
            res[str(n)] = case
            print(json.dumps(case), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
