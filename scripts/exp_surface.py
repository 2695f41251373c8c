"""Cost of the silhouette-refined surface mesh (vc_surface_mesh): (a) 128^3 and 1024^3 with the 4 real cameras and
the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p (ellipsoid masks with 0.5 % salt noise).  Per case and
step count (8, and 0 = topology and colour alone): surface_ms (HIP events around the whole call, median of the repetitions),
vertices, faces, refined, point_tests (camera tests evaluated) and tests per vertex.  At 1024^3 also the camera-order A/B
(option surface_order 1: the cameras that rejected P_off first, 0: camera order, alternated) and one photo_carve round of the
same hull for comparison.  --reps N (default 11), --quick (1024^3 only, 3 repetitions, no A/B: a profiler run), --out FILE
keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(eng, steps, reps, order=1):
    eng.set_option("surface_order", order)
    ms, st = [], None
    for _ in range(reps + 1):                                      # the first call allocates: left out
        st = eng.surface_mesh(steps)["stats"]
        ms.append(st["surface_ms"])
    eng.set_option("surface_order", 1)
    V = st["n_verts"]
    return {"steps": steps, "order": order, "surface_ms": float(np.median(ms[1:])), "min_ms": float(np.min(ms[1:])),
            "n_verts": V, "n_faces": st["n_faces"], "refined": st["refined"], "unrefined": st["unrefined"],
            "point_tests": st["point_tests"], "tests_per_vertex": st["point_tests"] / V if V else 0.0}


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import synthetic
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 11
    quick = "--quick" in sys.argv
    if quick:
        reps = 3
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n in ((1024,) if quick else (128, 1024)):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            for c, f in enumerate(frames):
                eng.upload_frame(c, f)
            case = {"grid": n, "cameras": 4, "survivors": eng.carve()}
            case["steps8"] = _time(eng, 8, reps)
            case["steps0"] = _time(eng, 0, reps)
            if n == 1024 and not quick:
                ab = {"first": [], "camera_order": []}
                for _ in range(3):                                 # alternated: other work shares the host
                    ab["first"].append(_time(eng, 8, max(reps // 3, 3), 1)["surface_ms"])
                    ab["camera_order"].append(_time(eng, 8, max(reps // 3, 3), 0)["surface_ms"])
                case["order_ab"] = {k: float(np.median(v)) for k, v in ab.items()}
                case["order_ab_tests"] = {"first": _time(eng, 8, 1, 1)["point_tests"], "camera_order": _time(eng, 8, 1, 0)["point_tests"]}
                case["photo_one_round_ms"] = eng.photo_carve(max_rounds=1)["photo_ms"]
            res[str(n)] = case
            print(json.dumps(case), flush=True)
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            case = {"grid": 512, "cameras": 16, "survivors": eng.carve()}
            case["steps8"] = _time(eng, 8, reps)
            case["steps0"] = _time(eng, 0, reps)
            res["config5"] = case
            print(json.dumps(case), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
