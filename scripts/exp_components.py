"""Cost of the connected-components pass (vc_hull_components) after a carve: the bench's workloads -- 1024^3 with the
4 real cameras and the committed MOG masks, config 5 (512^3, 16 ring cameras at 1080p, ellipsoid silhouettes with 0.5 % salt
noise) and 2048 x 2048 x 1023 with the real cameras.  Per configuration and connectivity: survivors before and after,
components, the largest, components_ms (HIP events around the whole call, median of the repetitions), the host clock around the
call; at 1024^3 also one vc_color_visible pass over the same hull for comparison.  Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/exp_components.py` for the kernels one by one; --out FILE keeps the
numbers as JSON.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _one(eng, grid, cams, masks, frames, reps, visible=False):
    H, W = masks[0].shape
    eng.set_grid(*grid)
    eng.set_cameras(cams, H, W)
    eng.upload_masks(masks)
    for c, f in enumerate(frames):
        eng.upload_frame(c, f)
    out = {"grid": list(grid), "cameras": len(cams), "image": [H, W]}
    if visible:
        vis = []
        for _ in range(3):
            eng.carve()
            eng.color_visible()
            vis.append(eng.timing()["visible_ms"])
        out["visible_ms"] = float(np.median(vis))
    for conn in (6, 18, 26):
        dev, host = [], []
        for k in range(reps + 2):
            eng.carve()
            t0 = time.perf_counter()
            st = eng.filter_components(connectivity=conn, keep_largest=1)
            t1 = time.perf_counter()
            if k >= 2:
                dev.append(st["components_ms"])
                host.append((t1 - t0) * 1e3)
        out["conn%d" % conn] = {"survivors_before": st["survivors_before"], "survivors_after": st["survivors_after"],
                                "components": st["components"], "largest": st["largest"],
                                "components_ms": float(np.median(dev)), "components_ms_min": float(np.min(dev)),
                                "host_call_ms": float(np.median(host))}
    return out


def main(out=None, reps=10, only=None):
    import voxcarve
    import fixtures_util as fx
    from voxcarve import synthetic
    res = {}
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(len(cams), *masks[0].shape)
    with voxcarve.CarveEngine(0) as eng:
        runs = [("real4_1024", lambda: _one(eng, (1024, 1024, 1024), cams, masks, frames, reps, visible=True))]
        H, W = 1080, 1920
        sc = synthetic.ring_cameras(16, H, W)
        runs.append(("config5_512", lambda: _one(eng, (512, 512, 512), sc, synthetic.ellipsoid_masks(sc, H, W),
                                                 synthetic.random_frames(16, H, W)[:2], reps)))
        runs.append(("real4_2048x2048x1023", lambda: _one(eng, (2048, 2048, 1023), cams, masks, frames, max(reps // 2, 1))))
        for name, f in runs:
            if only and name not in only:
                continue
            res[name] = f()
            print(json.dumps({name: res[name]}), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the numbers as JSON to this file")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="*", help="configuration names to run")
    a = ap.parse_args()
    main(a.out, a.reps, a.only)
