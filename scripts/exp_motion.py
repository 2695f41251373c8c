"""Cost of the block motion between two hulls and of the warp (vc_hull_motion, vc_hull_warp): (a) 128^3, 512^3 and
1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  A is the hull of the
masks as they are, B the hull of the masks rolled by ROLL columns (as tests/chain_model.py rolls them), kept in register 0.  Every
repetition runs, one after the other in the same process and on the same hull A:
  motion       hull_motion(0, b, a, s) for (8, 4, 4), the default, (4, 2, 2) and (16, 8, 8)
  warp         warp_hull(0, 1) after the default field
  components   vc_hull_components (connectivity 26, nothing removed): a pass that touches every survivor a few times
  compare_d    compare_hull(0, distance=True): the other pass that relates two hulls
Times are the calls' own HIP events (motion_ms, warp_ms, components_ms, compare_ms), medians with min and max of the repetitions
after a warm-up round.  --reps N (default 9), --quick (128^3 and 512^3 only, 3 repetitions), --out FILE keeps the numbers as JSON.
Needs an MI355X."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROLL = 9
PARAMS = ((8, 4, 4), (4, 2, 2), (16, 8, 8))


def _case(eng, grid, cameras, masks, reps):
    case = {"grid": grid, "cameras": cameras, "roll": ROLL}
    eng.upload_masks([np.ascontiguousarray(np.roll(m, ROLL, axis=1)) for m in masks])
    eng.carve(mode="fused")
    eng.keep_hull(0)
    case["survivors_b"] = eng.count
    eng.upload_masks(masks)
    eng.carve(mode="fused")
    case["survivors_a"] = eng.count
    rows = {}

    def note(name, ms):
        rows.setdefault(name, []).append(ms)

    for rep in range(reps + 1):                                    # round 0 allocates and warms up
        for b, a, s in PARAMS:
            st = eng.hull_motion(0, b, a, s)
            name = "motion_%d_%d_%d" % (b, a, s)
            if rep:
                note(name, st["motion_ms"])
            case.setdefault("stats", {})[name] = {k: v for k, v in st.items() if k != "motion_ms"}
        eng.hull_motion(0)
        w = eng.warp_hull(0, 1)
        cc = eng.filter_components(connectivity=26)
        cd = eng.compare_hull(0, distance=True)
        if rep:
            note("warp", w["warp_ms"])
            note("components", cc["components_ms"])
            note("compare_d", cd["compare_ms"])
    case["warp_stats"] = {k: v for k, v in w.items() if k != "warp_ms"}
    case["iou_before"] = cd["iou"]
    for name, v in rows.items():
        a = np.array(v)
        case[name] = {"ms": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    for name in ("components", "compare_d"):
        case["motion_8_4_4_over_" + name] = case["motion_8_4_4"]["ms"] / case[name]["ms"]
    return case


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import synthetic
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
    quick = "--quick" in sys.argv
    if quick:
        reps = 3
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n in ((128, 512) if quick else (128, 512, 1024)):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            eng.upload_frame(1, frames[1])
            res[str(n)] = _case(eng, n, 4, masks, reps)
            print(json.dumps(res[str(n)]), flush=True)
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            res["config5"] = _case(eng, 512, 16, rm, reps)
            print(json.dumps(res["config5"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
