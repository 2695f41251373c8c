"""Cost of the distance field of the hull and of the morphology built on it (vc_hull_distance, vc_hull_morphology):
(a) 128^3, 512^3 and 1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.
Per case, on the carve's result (mode="fused", min_views = all cameras): hull_distance inside only and with the outside field,
erode_hull and open_hull at 25 mm (a fresh carve in front of each: they change the result) -- distance_ms / morph_ms (HIP events
around the whole call) and the host's wall clock, medians of the repetitions after a warm-up call; then one call of each with
option timing_detail for the kernels' own times, the box and the lines.  Beside the times the traffic floor of the layout: a
transform over a box of B cells writes 8 B per cell along y and reads and writes 8 B per cell along x and along z, 40 B x B
(the outside field: B = N), divided by the 6.29 TB/s copy ceiling of DESIGN section 4.  --reps N (default 11), --quick
(1024^3 only, 3 repetitions: a profiler run), --out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING = 6.29e12          # bytes / s, the measured copy of DESIGN section 4
BYTES_PER_CELL = 40             # y: 8 written; x, z: 8 read + 8 written each
RADIUS_MM = 25.0


def _median(call, key, reps, before=None):
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates: left out
        if before:
            before()
        t0 = time.perf_counter()
        st = call()
        rows.append((st[key], (time.perf_counter() - t0) * 1e3))
    a = np.array(rows[1:])
    return st, {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "wall_ms": float(np.median(a[:, 1]))}


def _detail(eng, call, before=None):
    if before:
        before()
    eng.set_option("timing_detail", 1)
    eng.timing(reset=True)
    call()
    t = eng.timing()
    eng.set_option("timing_detail", 0)
    k = {name: v for name, v in t["kernels"].items() if name.startswith("k_dist")}
    return {"kernels": k, "cells": t["work"]["dist_cells"], "lines": t["work"]["dist_lines"]}


def _floor(row, cells):
    row["floor_bytes"] = BYTES_PER_CELL * cells
    row["floor_ms"] = row["floor_bytes"] / COPY_CEILING * 1e3
    row["fraction_of_floor"] = row["floor_ms"] / row["ms"]
    return row


def _case(eng, grid, cameras, reps):
    n = grid ** 3
    S = eng.carve(mode="fused")
    case = {"grid": grid, "cameras": cameras, "survivors": S}
    st, row = _median(lambda: eng.hull_distance(), "distance_ms", reps)
    box = st["sites_inside_box"] + st["survivors"]
    case["box_cells"], case["box_share_of_grid"] = box, box / n
    case["q_um"], case["max_depth_mm"] = st["q"], float(np.sqrt(float(st["max_d2"])) / 1000)
    case["inside"] = _floor(row, box)
    case["inside"]["detail"] = _detail(eng, lambda: eng.hull_distance())
    st, row = _median(lambda: eng.hull_distance(outside=True), "distance_ms", reps)
    case["inside_and_outside"] = _floor(row, box + n)
    case["inside_and_outside"]["detail"] = _detail(eng, lambda: eng.hull_distance(outside=True))
    carve = lambda: eng.carve(mode="fused")
    st, row = _median(lambda: eng.erode_hull(RADIUS_MM), "morph_ms", reps, before=carve)
    case["erode_25mm"] = _floor(row, box)
    case["erode_25mm"].update(eroded=st["eroded"], survivors_after=st["survivors_after"])
    st, row = _median(lambda: eng.open_hull(RADIUS_MM), "morph_ms", reps, before=carve)
    case["open_25mm"] = _floor(row, 2 * box)
    case["open_25mm"].update(eroded=st["eroded"], survivors_after=st["survivors_after"])
    case["open_25mm"]["detail"] = _detail(eng, lambda: eng.open_hull(RADIUS_MM), before=carve)
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
