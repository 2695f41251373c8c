"""Cost of occlusion-aware colouring (vc_color_visible) after a carve: the 4 real cameras and their masks at 128^3,
512^3 and 1024^3, and 16 synthetic cameras at 1080p at 512^3.  Per configuration: survivors, surface survivors, the pass's kernels
between two HIP events on the context's stream (vc_timing_t::visible_ms, median of the repetitions), the host clock around the
synchronous call, and the carve step of the same frame set for comparison (vc_timing_t::carve_ms + compact_ms of a vc_carve).
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/exp_visible.py` for the kernels one by one; --out FILE keeps the
numbers as JSON; --sweep times the two splat knobs too.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _one(eng, grid, cams, masks, frames, reps):
    H, W = masks[0].shape
    eng.set_grid(*grid)
    eng.set_cameras(cams, H, W)
    eng.upload_masks(masks)
    for c, f in enumerate(frames):
        eng.upload_frame(c, f)
    carve = []
    for _ in range(3):
        eng.touch_masks(0)
        S = eng.carve()
        t = eng.timing()
        carve.append(t["carve_ms"] + t["compact_ms"])
    dev, host = [], []
    for k in range(reps + 2):
        eng.carve()
        t0 = time.perf_counter()
        eng.color_visible()
        t1 = time.perf_counter()
        if k >= 2:
            dev.append(eng.timing()["visible_ms"])
            host.append((t1 - t0) * 1e3)
    surface = int((eng.fetch_visibility() != 0).sum())
    return {"grid": list(grid), "cameras": len(cams), "image": [H, W], "survivors": int(S), "visible_survivors": surface,
            "visible_ms": float(np.median(dev)), "visible_ms_min": float(np.min(dev)), "host_call_ms": float(np.median(host)),
            "carve_step_ms": float(np.median(carve))}


def _sweep(eng, key, grid, cams, masks, frames, reps, res):
    """The two splat knobs (vc_set_option visible_check, visible_big_rect) on one configuration."""
    for check in (1, 0):
        for big in (16, 64, 256, 1 << 30):
            eng.set_option("visible_check", check)
            eng.set_option("visible_big_rect", big)
            r = _one(eng, grid, cams, masks, frames, reps)
            res["%s_check%d_big%d" % (key, check, big)] = r["visible_ms"]
            print(key, "check", check, "big", big, round(r["visible_ms"], 4), flush=True)
    eng.set_option("visible_check", 1)
    eng.set_option("visible_big_rect", 64)


def main(out=None, reps=20, sweep=False):
    import voxcarve
    import fixtures_util as fx
    from voxcarve import synthetic
    res = {}
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    with voxcarve.CarveEngine(0) as eng:
        for n in (128, 512, 1024):
            res["real4_%d" % n] = _one(eng, (n, n, n), cams, masks, frames, reps)
            print(json.dumps(res["real4_%d" % n]), flush=True)
        H, W = 1080, 1920
        sc = synthetic.ring_cameras(16, H, W)
        sm, sf = synthetic.ellipsoid_masks(sc, H, W), synthetic.random_frames(16, H, W)
        res["synth16_1080p_512"] = _one(eng, (512, 512, 512), sc, sm, sf, reps)
        print(json.dumps(res["synth16_1080p_512"]), flush=True)
        if sweep:
            _sweep(eng, "real4_1024", (1024, 1024, 1024), cams, masks, frames, reps, res)
            _sweep(eng, "synth16_1080p_512", (512, 512, 512), sc, sm, sf, reps, res)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the numbers as JSON to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep", action="store_true", help="also time the splat knobs visible_check / visible_big_rect")
    a = ap.parse_args()
    main(a.out, a.reps, a.sweep)
