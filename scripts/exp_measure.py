"""Cost of measuring the hull's figures (vc_hull_measure) after a carve: (a) 128^3, 512^3 and 1024^3 with the 4 real
cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  Per case, on the carve's result
(mode="fused", min_views = all cameras): measure_ms (HIP events around the whole call: the output structs made, the sums, the
profile, the read-back) and the host's wall clock, medians of the repetitions after a warm-up call -- with one group (source
"all") and with the K = 4 figures of vc_hull_clusters as groups, each without and with the per-layer profile; and, for what the
host labels cost, 4096 groups handed in as an array (the upload of 4 B per record is inside the call).
The yardsticks, in the same run on the same hull: vc_hull_components with nothing removed (components_ms) and one
vc_color_visible pass (vc_timing_t::visible_ms); both are code this pass does not touch.  Beside the times what the pass must
move at the least: the records read once (8 B each, 9 B with the clusters' labels), over the 6.29 TB/s copy ceiling of DESIGN
section 4, and what fetching the records to do the sums on the host would move instead.
--reps N (default 11), --quick (1024^3 only, 3 repetitions: a profiler run), --out FILE keeps the numbers as JSON.
Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_CEILING = 6.29e12          # bytes / s, the measured copy of DESIGN section 4
K = 4


def _measure(eng, reps, **kw):
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates: left out
        t0 = time.perf_counter()
        st = eng.measure_hull(**kw)
        rows.append((st["measure_ms"], (time.perf_counter() - t0) * 1e3))
    a = np.array(rows[1:])
    return {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "wall_ms": float(np.median(a[:, 1])), "groups": st["groups"]}


def _components(eng, reps):
    dev = [eng.filter_components()["components_ms"] for _ in range(reps + 1)]      # min_voxels = 0: labels, removes nothing
    return {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}


def _visible(eng, reps):
    dev = []
    for _ in range(reps + 1):
        eng.timing(reset=True)
        eng.color_visible()
        dev.append(eng.timing()["visible_ms"])
    return {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}


def _case(eng, grid, cameras, reps):
    S = eng.carve(mode="fused")
    case = {"grid": grid, "cameras": cameras, "survivors": S, "k": K, "floor_bytes": 8 * S, "floor_ms": 8 * S / COPY_CEILING * 1e3,
            "fetch_bytes": 8 * S}
    case["all"] = _measure(eng, reps)
    case["all_profile"] = _measure(eng, reps, profile=True)
    eng.cluster_hull(K)
    case["clusters"] = _measure(eng, reps, labels="clusters")
    case["clusters_profile"] = _measure(eng, reps, labels="clusters", profile=True)
    lab = (np.arange(S, dtype=np.int64) * 2654435761 % 4096).astype(np.uint32)
    case["host_4096"] = _measure(eng, max(reps // 3, 1), labels=lab, groups=4096)
    from voxcarve import measure
    w = measure.describe(eng.fetch_measure(), eng.grid, eng.bounds)
    case["all_volume_mm3"] = float(measure.describe(_all(eng), eng.grid, eng.bounds)["volume_mm3"][0])
    case["host_4096_volume_mm3"] = float(w["volume_mm3"].sum())
    case["hull_components"] = _components(eng, reps)
    case["color_visible"] = _visible(eng, reps)
    for k in ("all", "clusters", "clusters_profile"):
        case[k + "_over_hull_components"] = case[k]["ms"] / case["hull_components"]["ms"]
        case[k + "_over_color_visible"] = case[k]["ms"] / case["color_visible"]["ms"]
    return case


def _all(eng):
    eng.measure_hull()
    return eng.fetch_measure()


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
            for c in range(4):
                eng.upload_frame(c, frames[c])
            res[str(n)] = _case(eng, n, 4, reps)
            print(json.dumps(res[str(n)]), flush=True)
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
            res["config5"] = _case(eng, 512, 16, reps)
            print(json.dumps(res["config5"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
