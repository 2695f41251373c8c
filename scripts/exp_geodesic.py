"""Cost of the geodesic distances through the hull and its extremities (vc_hull_geodesic) after a carve: (a) 128^3,
512^3 and 1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  Per case,
on the carve's result (mode="fused", min_views = all cameras), seeds = the floor layer, connectivity 26, K = 5: geodesic_ms (HIP
events around the whole call: the words' record offsets, the survivors' box, the seeds, the relaxations with their read-backs, the
two arg-max passes per extremity) and the host's wall clock, medians of the repetitions after a warm-up call, with rounds,
launches and tile visits -- on the tile route (vc_set_option "geodesic_tiles" = 1) and on the sweep route (= 0; it takes seconds
at the large sizes, so it gets at most --sweep-reps repetitions there).  The same with K = 0 says what the first relaxation costs;
warm_share = (K = 5 minus K = 0) over K = 5 is the share of the 5 warm-started re-relaxations and their arg-max passes.  With
paths=True the five walks back are in it too.  The yardsticks, in the same run on the same hull: vc_hull_components (26, nothing
removed) and vc_hull_distance (inside field); both are code this pass does not touch.
--reps N (default 11), --sweep-reps N (default 2), --quick (1024^3 only, 3 repetitions, one of the sweep route: a profiler run),
--out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = 5


def _geodesic(eng, reps, extrema=K, paths=False):
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates: left out
        t0 = time.perf_counter()
        st = eng.hull_geodesic(seeds="floor", extrema=extrema, connectivity=26, paths=paths)
        rows.append((st["geodesic_ms"], (time.perf_counter() - t0) * 1e3))
    a = np.array(rows[1:])
    return st, {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "wall_ms": float(np.median(a[:, 1])),
                "rounds": st["rounds"], "launches": st["launches"], "tile_visits": st["tile_visits"], "repetitions": reps}


def _route(eng, reps, with_paths):
    _, first = _geodesic(eng, reps, extrema=0)
    st, full = _geodesic(eng, reps)                                # (last, so that the keys left behind are those of K extremities)
    out = {"k5": full, "k0": first, "warm_share": (full["ms"] - first["ms"]) / full["ms"] if full["ms"] > 0 else 0.0}
    if with_paths:
        _, out["k5_with_paths"] = _geodesic(eng, reps, paths=True)
    return st, out


def _case(eng, grid, cameras, reps, sweep_reps):
    S = eng.carve(mode="fused")
    eng.set_option("geodesic_tiles", 1)
    st, tiles = _route(eng, reps, True)
    d_tiles, l_tiles = eng.fetch_geodesic(), eng.fetch_geodesic_labels()
    case = {"grid": grid, "cameras": cameras, "survivors": S, "seeds": st["seeds"], "reached": st["reached"], "k": K, "q_um": st["q"],
            "edge_um": st["edge_um"], "tiles_in_box": st["tiles"], "extremities": st["extremities"], "max_d_um": st["max_d"],
            "extrema_d_um": eng.fetch_extrema()["d"].tolist(), "tiles": tiles}
    eng.set_option("geodesic_tiles", 0)
    try:
        _, case["sweeps"] = _route(eng, reps if grid < 512 else min(reps, sweep_reps), False)
        case["routes_equal"] = bool(np.array_equal(d_tiles, eng.fetch_geodesic()) and np.array_equal(l_tiles, eng.fetch_geodesic_labels()))
    finally:
        eng.set_option("geodesic_tiles", 1)
    dev = [eng.filter_components(connectivity=26)["components_ms"] for _ in range(reps + 1)]      # labels, removes nothing
    case["hull_components"] = {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}
    dev = [eng.hull_distance()["distance_ms"] for _ in range(reps + 1)]
    case["hull_distance"] = {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}
    case["tiles_over_sweeps"] = tiles["k5"]["ms"] / case["sweeps"]["k5"]["ms"]
    case["tiles_over_hull_components"] = tiles["k5"]["ms"] / case["hull_components"]["ms"]
    case["tiles_over_hull_distance"] = tiles["k5"]["ms"] / case["hull_distance"]["ms"]
    return case


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import synthetic
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 11
    sweep_reps = int(sys.argv[sys.argv.index("--sweep-reps") + 1]) if "--sweep-reps" in sys.argv else 2
    quick = "--quick" in sys.argv
    if quick:
        reps, sweep_reps = 3, 1
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    res = {}

    def keep():
        if out_path:
            with open(out_path, "w") as f:
                json.dump(res, f, indent=1)

    with voxcarve.CarveEngine(0) as eng:
        for n in ((1024,) if quick else (128, 512, 1024)):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            for c in range(4):
                eng.upload_frame(c, frames[c])
            res[str(n)] = _case(eng, n, 4, reps, sweep_reps)
            print(json.dumps(res[str(n)]), flush=True)
            keep()
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            rf = [np.random.default_rng(3000 + c).integers(0, 256, (H, W, 3), dtype=np.uint8) for c in range(16)]
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            for c in range(16):
                eng.upload_frame(c, rf[c])
            res["config5"] = _case(eng, 512, 16, reps, sweep_reps)
            print(json.dumps(res["config5"]), flush=True)
            keep()


if __name__ == "__main__":
    main()
