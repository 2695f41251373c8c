"""Cost of the vote over the last frames' hulls (vc_hull_temporal): (a) 128^3, 512^3 and 1024^3 with the 4 real cameras
and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  Every frame's masks carry the seeded noise of the
design's recipe (2 % of each mask's pixels flipped, generator 7000 + t), so the vote restores and drops voxels as it does on
video.  Per case and per window (3, 5, 15, majority vote): the ring is filled, then every repetition carves the next noisy frame
(mode="fused", min_views = all cameras) and votes -- temporal_ms (HIP events around the whole call, two device-to-device copies of
the occupancy words included) and the host's wall clock, medians of the repetitions; beside it filter_components on the same
voted hull, the yardstick the other passes use; then one call with option timing_detail for the kernels' own times, from which the
vote kernel's achieved bytes/s follow: it reads the m - 1 older snapshots, the current words and P and writes O, (m + 3) nwords 8
bytes at m = window.  (A profiler's kernel times replace the events' where a trace was taken: --quick.)
--reps N (default 11), --quick (1024^3 with window 5 only, 3 repetitions: a profiler run), --out FILE keeps the numbers as JSON.
Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOWS = (3, 5, 15)
NOISE = 0.02
SETS = 4            # noisy mask sets made once per case and cycled through


def _noisy(masks, t):
    rng = np.random.default_rng(7000 + t)
    return [np.where(rng.random(m.shape) < NOISE, 255 - m, m).astype(np.uint8) for m in masks]


def _case(eng, grid, cameras, sets, reps, windows):
    nwords = (grid ** 3 + 63) // 64
    case = {"grid": grid, "cameras": cameras, "nwords": nwords}
    frame = [0]

    def carve():
        eng.upload_masks(sets[frame[0] % len(sets)])
        frame[0] += 1
        return eng.carve(mode="fused")

    for window in windows:
        eng.temporal_reset()
        for _ in range(window + 1):                                # fills the ring; the first call allocates
            carve()
            st = eng.temporal_filter(window)
        rows = []
        for _ in range(reps):
            carve()
            t0 = time.perf_counter()
            st = eng.temporal_filter(window)
            wall = (time.perf_counter() - t0) * 1e3
            cc = eng.filter_components(min_voxels=1)
            rows.append((st["temporal_ms"], wall, cc["components_ms"]))
        a = np.array(rows)
        row = {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "wall_ms": float(np.median(a[:, 1])),
               "components_ms": float(np.median(a[:, 2]))}
        row.update({k: v for k, v in st.items() if k != "temporal_ms"})
        carve()
        eng.set_option("timing_detail", 1)
        eng.timing(reset=True)
        eng.temporal_filter(window)
        k = eng.timing()["kernels"]
        eng.set_option("timing_detail", 0)
        row["kernels"] = {name: v for name, v in k.items() if "temporal" in name}
        vote_ms = k["k_temporal_vote"]["ms_sum"]
        row["vote_bytes"] = (window + 3) * nwords * 8
        row["vote_tb_per_s"] = row["vote_bytes"] / (vote_ms * 1e-3) / 1e12 if vote_ms > 0 else None
        case["window_%d" % window] = row
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
    windows = (5,) if quick else WINDOWS
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    sets = [_noisy(masks, t) for t in range(SETS)]
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n in ((1024,) if quick else (128, 512, 1024)):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            eng.upload_frame(1, frames[1])
            res[str(n)] = _case(eng, n, 4, sets, reps, windows)
            print(json.dumps(res[str(n)]), flush=True)
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            rsets = [_noisy(rm, t) for t in range(SETS)]
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            res["config5"] = _case(eng, 512, 16, rsets, reps, windows)
            print(json.dumps(res["config5"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
