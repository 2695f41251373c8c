"""Cost of the footprint carve (vc_carve_footprint) next to the centre carve in mode="fused" on the same inputs and
device: (a) 128^3 and 1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at
1080p (ellipsoid masks with 0.5 % salt noise).  Masks resident, min_views = all cameras.  Per case and rule ("any", "all"):
carve_ms (HIP events around the carve kernel), compact_ms (counts, scan, record expansion), their sum and the host's wall
clock of the whole call, medians of the repetitions after a warm-up call; then one call with option timing_detail for the work
counters (projections, words, word-camera visits the union test ended) and the table build, timed apart by touching the masks.
The centre carve's path is the one the parent commit has (this rule does not touch it).  --reps N (default 11), --quick
(1024^3 only, 3 repetitions: a profiler run), --out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(eng, reps, **kw):
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates (and builds the table): left out
        t0 = time.perf_counter()
        n = eng.carve(**kw)
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.timing()
        rows.append((t["carve_ms"], t["compact_ms"], t["carve_ms"] + t["compact_ms"], wall))
    a = np.array(rows[1:])
    med = np.median(a, axis=0)
    return {"survivors": n, "carve_ms": float(med[0]), "compact_ms": float(med[1]), "device_ms": float(med[2]), "wall_ms": float(med[3]),
            "device_ms_min": float(a[:, 2].min())}


def _detail(eng, rule, voxels, cameras):
    eng.set_option("timing_detail", 1)
    eng.touch_masks(0)                                             # the slot is prepared again: the table is rebuilt
    eng.timing(reset=True)
    eng.carve(footprint=rule)
    t = eng.timing()
    eng.set_option("timing_detail", 0)
    w = t["work"]
    words = w["foot_words"]
    return {"table_build_ms": t["kernels"].get("foot_table", {}).get("ms_sum", 0.0), "carve_kernel_ms": t["kernels"]["k_carve_foot"]["ms_sum"],
            "projections": w["foot_projections"], "projections_per_voxel": w["foot_projections"] / voxels,
            "words": words, "union_skips": w["foot_union_skips"], "union_skips_per_word": w["foot_union_skips"] / words,
            "share_of_word_camera_visits_skipped": w["foot_union_skips"] / (words * cameras)}


def _case(eng, grid, cameras, reps):
    n = grid ** 3
    case = {"grid": grid, "cameras": cameras, "centre_fused": _time(eng, reps, mode="fused")}
    for rule in ("any", "all"):
        case[rule] = _time(eng, reps, footprint=rule)
        case[rule]["detail"] = _detail(eng, rule, n, cameras)
    case["any_over_centre"] = case["any"]["device_ms"] / case["centre_fused"]["device_ms"]
    return case


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
            eng.upload_frame(1, frames[1])
            res[str(n)] = _case(eng, n, 4, reps)
            print(json.dumps(res[str(n)]), flush=True)
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            res["config5"] = _case(eng, 512, 16, reps)
            print(json.dumps(res["config5"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
