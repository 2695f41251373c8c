"""Cost of photo-consistency carving (vc_photo_carve) after a carve, on the textured pit scene
(synthetic.textured_scene): the 4 real cameras at 256^3, 512^3 and 1024^3 (a 700 x 700 x 600 mm block with a 400 x 400 x 150 mm
pit standing on the floor in front of them, default bounds), and 16 ring cameras at 1080p at 512^3 (the default block at the
volume centre).  Per configuration: survivors before and after, rounds, whether the loop converged, photo_ms (HIP events around
the whole call, median of the repetitions), ms per round, the host clock around the call, and one vc_color_visible pass over the
visual hull of the same frame set for comparison (vc_timing_t::visible_ms).  Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/exp_photo.py` for the kernels one by one (the compaction is
k_compact_count<PhotoKept>, k_scan_groups / k_scan_blocks and k_compact_scatter<PhotoKept>); --out FILE keeps the numbers as JSON.
Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REAL_PIT = dict(centre=(360.0, 40.0, -300.0), half=(350.0, 350.0, 300.0), opening=(200.0, 200.0), depth=150.0)


def _one(eng, grid, cams, masks, frames, reps, max_rounds=64):
    H, W = masks[0].shape
    eng.set_grid(*grid)
    eng.set_cameras(cams, H, W)
    eng.upload_masks(masks)
    for c, f in enumerate(frames):
        eng.upload_frame(c, f)
    vis = []
    for _ in range(3):
        eng.carve()
        eng.color_visible()
        vis.append(eng.timing()["visible_ms"])
    dev, host = [], []
    for k in range(reps + 2):
        eng.carve()
        t0 = time.perf_counter()
        st = eng.photo_carve(max_rounds=max_rounds)
        t1 = time.perf_counter()
        if k >= 2:
            dev.append(st["photo_ms"])
            host.append((t1 - t0) * 1e3)
    ms = float(np.median(dev))
    return {"grid": list(grid), "cameras": len(cams), "image": [H, W], "survivors_before": st["survivors_before"],
            "survivors_after": st["survivors_after"], "rounds": st["rounds"], "converged": st["converged"],
            "photo_ms": ms, "photo_ms_min": float(np.min(dev)), "ms_per_round": ms / st["rounds"],
            "host_call_ms": float(np.median(host)), "visible_ms_visual_hull": float(np.median(vis))}


def main(out=None, reps=10):
    import voxcarve
    import fixtures_util as fx
    from voxcarve import synthetic
    res = {}
    cams = fx.golden_cameras()
    H, W = 486, 644
    masks, frames = synthetic.textured_scene(cams, H, W, **REAL_PIT)
    with voxcarve.CarveEngine(0) as eng:
        for n in (256, 512, 1024):
            res["real4_pit_%d" % n] = _one(eng, (n, n, n), cams, masks, frames, reps)
            print(json.dumps(res["real4_pit_%d" % n]), flush=True)
        H, W = 1080, 1920
        sc = synthetic.ring_cameras(16, H, W)
        sm, sf = synthetic.textured_scene(sc, H, W)
        res["ring16_1080p_pit_512"] = _one(eng, (512, 512, 512), sc, sm, sf, reps)
        print(json.dumps(res["ring16_1080p_pit_512"]), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the numbers as JSON to this file")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    main(a.out, a.reps)
