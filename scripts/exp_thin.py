"""Cost of thinning the hull to a skeleton (vc_hull_thin) after a carve: (a) 128^3, 512^3 and 1024^3 with the 4 real
cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  Per case, on the carve's result
(mode="fused", min_views = all cameras), for both modes ("curve", "point") and both routes of the predicate (option thin_table =
0: in registers, 1: by look-up): thin_ms (HIP events around the whole call) and the host's wall clock, medians of the repetitions
after a warm-up call, with the passes, the direction steps that had a candidate, the launches and the kept voxels.  One more call
per mode and route runs with option timing_detail = 1, where every kernel carries its own begin / end events: thin_kernel_ms is
their sum and 1 - thin_kernel_ms / thin_ms the share of the call the stream spent between kernels (the events themselves cost
the stream some time, so thin_ms of that call is given beside it and is not the figure to quote).
The yardsticks, in the same run on the same hull: vc_hull_components with nothing removed (components_ms) and vc_hull_distance
(distance_ms); both are code this pass does not touch.
Every workload runs in a child process of its own (--case NAME: 128, 512, 1024 or config5, in this process) under a time limit;
the first that fails ends the run.
--reps N (default 5), --quick (1024^3, "curve", 2 repetitions: a profiler run), --out FILE keeps the numbers as JSON.
Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEEP = ("kept", "passes", "steps", "launches", "stable", "endpoints", "junctions")


def _thin(eng, reps, mode, route):
    eng.set_option("thin_table", route)
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates (and builds the table): left out
        t0 = time.perf_counter()
        st = eng.thin_hull(mode)
        rows.append((st["thin_ms"], (time.perf_counter() - t0) * 1e3))
    a = np.array(rows[1:])
    out = {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "ms_max": float(a[:, 0].max()),
           "wall_ms": float(np.median(a[:, 1]))}
    out.update({k: st[k] for k in KEEP})
    eng.set_option("timing_detail", 1)
    try:
        st = eng.thin_hull(mode)
        t = eng.timing()
    finally:
        eng.set_option("timing_detail", 0)
        eng.set_option("thin_table", 0)
    out["detail"] = {"thin_ms": st["thin_ms"], "thin_kernel_ms": t["thin_kernel_ms"], "kernels_timed": t["thin_launches"],
                     "between_kernels_share": 1.0 - t["thin_kernel_ms"] / st["thin_ms"] if st["thin_ms"] > 0 else 0.0}
    return out


def _components(eng, reps):
    dev = [eng.filter_components()["components_ms"] for _ in range(reps + 1)]      # min_voxels = 0: labels, removes nothing
    return {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}


def _distance(eng, reps):
    dev = [eng.hull_distance()["distance_ms"] for _ in range(reps + 1)]
    return {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}


def _case(eng, grid, cameras, reps, modes):
    S = eng.carve(mode="fused")
    case = {"grid": grid, "cameras": cameras, "survivors": S}
    for mode in modes:
        for route in (0, 1):
            case["%s_table%d" % (mode, route)] = _thin(eng, reps, mode, route)
        case[mode + "_table_over_registers"] = case[mode + "_table1"]["ms"] / case[mode + "_table0"]["ms"]
    case["hull_components"] = _components(eng, reps)
    case["hull_distance"] = _distance(eng, reps)
    for mode in modes:
        case[mode + "_over_hull_components"] = case[mode + "_table0"]["ms"] / case["hull_components"]["ms"]
        case[mode + "_over_hull_distance"] = case[mode + "_table0"]["ms"] / case["hull_distance"]["ms"]
    return case


CASES = ("128", "512", "1024", "config5")
CASE_SECONDS = 300              # the limit of one case's process


def _run_case(name, reps, modes):
    """One workload in this process."""
    import fixtures_util as fx
    import voxcarve
    from voxcarve import synthetic
    with voxcarve.CarveEngine(0) as eng:
        if name == "config5":
            H, W = 1080, 1920
            cams = synthetic.ring_cameras(16, H, W)
            masks = synthetic.ellipsoid_masks(cams, H, W)
            frames = [np.random.default_rng(3000 + c).integers(0, 256, (H, W, 3), dtype=np.uint8) for c in range(16)]
            n = 512
        else:
            cams, masks = fx.golden_cameras(), fx.golden_masks()
            H, W = masks[0].shape
            frames = fx.synthetic_frames(4, H, W)
            n = int(name)
        eng.set_grid(n, n, n)
        eng.set_cameras(cams, H, W)
        eng.upload_masks(masks)
        for c in range(len(cams)):
            eng.upload_frame(c, frames[c])
        return _case(eng, n, len(cams), reps, modes)


def main():
    """Without --case: every workload in a child process of its own, under its own time limit, one after the other; the first
    that fails or runs out of time ends the run (nothing more is started on the device) and what was measured so far is kept."""
    import subprocess
    import tempfile
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    quick = "--quick" in sys.argv
    modes = ("curve",) if quick else ("curve", "point")
    if quick:
        reps = 2
    if "--case" in sys.argv:
        name = sys.argv[sys.argv.index("--case") + 1]
        res = {name: _run_case(name, reps, modes)}
        print(json.dumps(res[name]), flush=True)
    else:
        res = {}
        for name in (("1024",) if quick else CASES):
            with tempfile.TemporaryDirectory() as tmp:
                part = os.path.join(tmp, "case.json")
                cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(reps), "--out", part] + (["--quick"] if quick else [])
                try:
                    code = subprocess.run(cmd, timeout=CASE_SECONDS).returncode
                except subprocess.TimeoutExpired:
                    code = 124
                if code == 0:
                    res.update(json.load(open(part)))
            if out_path:
                with open(out_path, "w") as f:
                    json.dump(res, f, indent=1)
            if code != 0:
                sys.exit("case %s ended with status %d: stopped there" % (name, code))
        return
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
