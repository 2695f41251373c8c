"""Cost of the growing half of the hull's morphology (vc_hull_grow) beside the opening it mirrors: (a) 128^3, 512^3
and 1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  Per case, on the
carve's result (mode="fused", min_views = all cameras): dilate_hull, close_hull and open_hull at 25 mm, a fresh carve in front
of every call (they change the result) -- grow_ms / morph_ms (HIP events around the whole call) and the host's wall clock, medians
of the repetitions after a warm-up call; then one call of each with option timing_detail for the kernels' own times, the box and
the lines.  open_hull is the yardstick: the closing runs the same two transforms over a box a few cells larger, plus the merge.
--reps N (default 11), --quick (1024^3 only, 3 repetitions: a profiler run), --out FILE keeps the numbers as JSON.  Needs an
MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RADIUS_MM = 25.0


def _median(call, key, reps, before):
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates: left out
        before()
        t0 = time.perf_counter()
        st = call()
        rows.append((st[key], (time.perf_counter() - t0) * 1e3))
    a = np.array(rows[1:])
    return st, {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "wall_ms": float(np.median(a[:, 1]))}


def _detail(eng, call, before):
    before()
    eng.set_option("timing_detail", 1)
    eng.timing(reset=True)
    call()
    t = eng.timing()
    eng.set_option("timing_detail", 0)
    k = {name: v for name, v in t["kernels"].items() if name.startswith("k_dist") or "grow" in name}
    return {"kernels": k, "cells": t["work"]["dist_cells"], "lines": t["work"]["dist_lines"]}


def _case(eng, grid, cameras, reps):
    n = grid ** 3
    carve = lambda: eng.carve(mode="fused")
    case = {"grid": grid, "cameras": cameras, "survivors": carve()}
    for name, call, key in (("dilate_25mm", lambda: eng.dilate_hull(RADIUS_MM), "grow_ms"),
                            ("close_25mm", lambda: eng.close_hull(RADIUS_MM), "grow_ms"),
                            ("open_25mm", lambda: eng.open_hull(RADIUS_MM), "morph_ms")):
        st, row = _median(call, key, reps, carve)
        row.update({k: v for k, v in st.items() if k not in ("grow_ms", "morph_ms")})
        if "box_cells" in st:
            row["box_share_of_grid"] = st["box_cells"] / n
        row["detail"] = _detail(eng, call, carve)
        case[name] = row
    case["close_over_open"] = case["close_25mm"]["ms"] / case["open_25mm"]["ms"]
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
        for n in ((1024,) if quick else (128, 512, 1024)):
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
