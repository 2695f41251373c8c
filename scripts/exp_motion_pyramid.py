"""Cost and gain of the coarse-to-fine block motion (vc_hull_motion_pyramid) beside the single-level field: (a) 128^3,
512^3 and 1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  A is the hull
of the masks as they are, B the hull of the masks rolled by ROLL columns, kept in register 0: the hull pair of scripts/exp_motion.py.
Every repetition runs, one after the other in the same process and on the same hull A, at block 8, apron 4, search 4:
  single       hull_motion(0, 8, 4, 4): the yardstick, the kernels vc_hull_motion has always run
  L<l>_r<r>    hull_motion(0, 8, 4, 4, levels=l, refine=r) for l in 1, 2, 3 and r in 1, 2
each followed once (in the warm-up round) by warp_hull(0, 1) for predicted_iou.  Times are the calls' own HIP events (motion_ms),
medians with min and max of the repetitions after a warm-up round; beside them the ratio to the yardstick, clipped, borrowed,
cost_sum / cost0_sum and the displacements tried.  --reps N (default 9), --quick (128^3 and 512^3 only, 3 repetitions), --out FILE
keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROLL = 9
BLOCK, APRON, SEARCH = 8, 4, 4
ROUTES = [("single", 0, 1)] + [("L%d_r%d" % (l, r), l, r) for l in (1, 2, 3) for r in (1, 2)]


def _case(eng, grid, cameras, masks, reps):
    case = {"grid": grid, "cameras": cameras, "roll": ROLL, "block": BLOCK, "apron": APRON, "search": SEARCH}
    eng.upload_masks([np.ascontiguousarray(np.roll(m, ROLL, axis=1)) for m in masks])
    eng.carve(mode="fused")
    eng.keep_hull(0)
    case["survivors_b"] = eng.count
    eng.upload_masks(masks)
    eng.carve(mode="fused")
    case["survivors_a"] = eng.count
    case["iou_before"] = eng.compare_hull(0)["iou"]
    times = {}
    for rep in range(reps + 1):                                    # round 0 allocates, warms up and warps
        for name, levels, refine in ROUTES:
            st = eng.hull_motion(0, BLOCK, APRON, SEARCH, levels=levels, refine=refine)
            if rep:
                times.setdefault(name, []).append(st["motion_ms"])
                continue
            row = {k: v for k, v in st.items() if k != "motion_ms"}
            row["cost_ratio"] = st["cost_sum"] / st["cost0_sum"] if st["cost0_sum"] else None
            row["predicted_iou"] = eng.warp_hull(0, 1)["predicted_iou"]
            case[name] = row
    for name, v in times.items():
        a = np.array(v)
        case[name].update(ms=float(np.median(a)), ms_min=float(a.min()), ms_max=float(a.max()))
    for name, _, _ in ROUTES:
        case[name]["over_single"] = case[name]["ms"] / case["single"]["ms"]
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

    def keep():
        if out_path:
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)

    with voxcarve.CarveEngine(0) as eng:
        for n in ((128, 512) if quick else (128, 512, 1024)):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            eng.upload_frame(1, frames[1])
            res[str(n)] = _case(eng, n, 4, masks, reps)
            print(json.dumps(res[str(n)]), flush=True)
            keep()
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            res["config5"] = _case(eng, 512, 16, rm, reps)
            print(json.dumps(res["config5"]), flush=True)
            keep()


if __name__ == "__main__":
    main()
