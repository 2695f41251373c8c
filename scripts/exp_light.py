"""Cost of the lit pass (vc_light_render) with the 4 real cameras and the committed MOG masks: 128^3 seen by the 4
calibrated cameras at their own 486 x 644, and 1024^3 seen by 8 orbit views at 1080p.  Per case light_ms (HIP events around the
whole call, median of the repetitions) with the floor and without it, at ao_reach 4 and at 0 (shadow rays only), the contract's
counts and the walk's diagnostics, beside the two yardsticks on the same images: render_ms of the vc_render the pass follows, and
the vc_shade_render of the same images.  vc_shade_render reports no time of its own, so it is timed by the host clock around the
call, which ends in a stream synchronise; light_wall_ms is the lit pass on the same clock.  The ratios light / render and light /
shade use like for like (events against events, host clock against host clock).  --reps N (default 11), --quick (3 repetitions),
--out FILE keeps the numbers as JSON.  Needs an MI355X."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _light(eng, lighting, pos, floor, ao_reach, reps):
    """The pass alone (no fetch of its images): events and host clock, medians over `reps` calls after one that allocates."""
    L = lighting.light_struct(pos, 64, False, ao_reach, floor, eng.grid, eng.bounds)
    st = lighting.LightStats()
    ms, wall = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        eng._check(eng._L.vc_light_render(eng._ctx, ctypes.byref(L), 0, ctypes.byref(st)), "vc_light_render")
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(st.light_ms))
    out = {name: int(getattr(st, name)) for name, _ in st._fields_ if name != "light_ms"}
    out.update(floor=floor is not None, ao_reach=ao_reach, light_ms=float(np.median(ms[1:])), min_ms=float(np.min(ms[1:])),
               light_wall_ms=float(np.median(wall[1:])))
    cast = out["rays_walked"]
    out["cells_per_ray"] = out["cells_visited"] / cast if cast else 0.0
    return out


def _shade_wall(eng, views, reps):
    light = np.ascontiguousarray([-np.asarray(v.R, dtype=np.float64).reshape(3, 3)[2, :] for v in views])
    wall = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        eng._check(eng._L.vc_shade_render(eng._ctx, light.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 64, 0), "vc_shade_render")
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall[1:]))


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import camera, lighting
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 11
    if "--quick" in sys.argv:
        reps = 3
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    cases = {128: ("cameras_486x644", cams, H0, W0), 1024: ("orbit_1080p", camera.orbit(8, 4500.0, 25.0, 1500.0, 1080, 1920), 1080, 1920)}
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n, (name, views, H, W) in cases.items():
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            for c, f in enumerate(frames):
                eng.upload_frame(c, f)
            case = {"grid": n, "views": name, "n_views": len(views), "H": H, "W": W, "survivors": eng.carve()}
            eng.hull_normals()
            rs = [eng.render(views, H, W)["stats"] for _ in range(reps + 1)]
            case["render_ms"] = float(np.median([s["render_ms"] for s in rs[1:]]))
            case["render_hits"], case["render_cells"] = rs[-1]["hits"], rs[-1]["cells_visited"]
            case["shade_wall_ms"] = _shade_wall(eng, views, reps)
            pos = lighting.light_above(views[0])
            auto = lighting.auto_floor(eng.grid, eng.bounds)
            case["floor_ao4"] = _light(eng, lighting, pos, auto, 4.0, reps)
            case["hull_ao4"] = _light(eng, lighting, pos, None, 4.0, reps)
            case["hull_ao0"] = _light(eng, lighting, pos, None, 0.0, reps)
            for k in ("floor_ao4", "hull_ao4", "hull_ao0"):
                case[k]["light_over_render"] = case[k]["light_ms"] / case["render_ms"]
                case[k]["light_over_shade"] = case[k]["light_wall_ms"] / case["shade_wall_ms"]
            res[str(n)] = case
            print(json.dumps(case), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
