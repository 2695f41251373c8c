"""Cost of the contour stage on the device: vc_fill_figures at 486 x 644 and 1080p, vc_foreground_to_slot with
4 cameras at 486 x 644, and the host path it replaces per frame set (vc_foreground_front, mask down, mask up).  Host clock
around calls that end in a device synchronise; run it under `rocprofv3 --kernel-trace --stats -- python scripts/exp_fill.py`
for the kernels' own times; --out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main(out=None):
    import voxcarve
    import contour_masks as cm
    import fixtures_util as fx
    from voxcarve import background_subtraction as bs
    from voxcarve.assignment import cam_bg_model_params
    rng = np.random.default_rng(0)
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for H, W in ((486, 644), (1080, 1920)):
            m = cm.blobs(rng, H, W, k=max(H, W) // 16)
            res["fill_figures_%dx%d_ms" % (H, W)] = _median_ms(lambda: eng.fill_figures(m, 5000, 115))
        masks = fx.golden_masks()
        res["fill_figures_golden_mask_ms"] = _median_ms(lambda: eng.fill_figures(masks[0], 5000, 115))
        H, W = masks[0].shape
        frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
        models = [bs.train_MOG_background_model(history=4, n_mixtures=50, bg_ratio=0.9, frames=[f] * 4, engine=eng) for f in frames]
        eng.set_grid(128, 128, 128)
        eng.set_cameras(fx.golden_cameras(), H, W)

        def device_path():
            eng.foreground_to_slot(models, frames, cam_bg_model_params, slot=0)
            eng.synchronize()
        res["foreground_to_slot_4cams_ms"] = _median_ms(device_path)

        def host_path():                        # what the cv2 stage needs around it: front half down, masks back up
            ms = [eng.foreground_front(models[c]._model, frames[c], 0, *cam_bg_model_params[c][2:4]) for c in range(4)]
            eng.upload_masks(ms, slot=1)
            for c in range(4):
                eng.upload_frame(c, frames[c], slot=1)
            eng.synchronize()
        res["host_path_front_down_up_4cams_ms"] = _median_ms(host_path)
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the numbers as JSON to this file")
    main(ap.parse_args().out)
