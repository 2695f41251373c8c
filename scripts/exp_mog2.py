"""Cost of the MOG2 background model on the device: vc_mog2_apply and vc_foreground_front with a MOG2 model per frame
at 486 x 644 and 1080p (host buffers in and out), and vc_foreground_to_slot with four MOG2 cameras at 486 x 644.  Host clock
around calls that end in a device synchronise; run it under `rocprofv3 --kernel-trace --stats -- python scripts/exp_mog2.py` for
the kernels' own times; --out FILE keeps the numbers as JSON.  Needs an MI355X."""
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


def _background(rng, H, W, n):
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return [np.clip(bg.astype(np.int16) + rng.integers(-5, 6, bg.shape), 0, 255).astype(np.uint8) for _ in range(n)]


def main(out=None):
    import voxcarve
    import fixtures_util as fx
    from voxcarve import background_subtraction as bs
    from voxcarve.assignment import cam_bg_model_params
    rng = np.random.default_rng(0)
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for H, W in ((486, 644), (1080, 1920)):
            frames = _background(rng, H, W, 8)
            model = bs.train_MOG2_background_model(history=32, frames=frames * 4, engine=eng)
            nmodes = model.state()[1]
            res["mog2_mean_nmodes_%dx%d" % (H, W)] = float(nmodes.mean())
            k = [0]

            def apply():
                k[0] += 1
                eng.mog2_apply(model._model, frames[k[0] % 8], 0)
            res["mog2_apply_%dx%d_ms" % (H, W)] = _median_ms(apply)
            res["foreground_front_mog2_%dx%d_ms" % (H, W)] = _median_ms(
                lambda: eng.foreground_front(model._model, frames[3], 0, True, True))
            model.close()
        masks = fx.golden_masks()
        H, W = masks[0].shape
        bgs = [_background(rng, H, W, 4) for _ in range(4)]
        models = [bs.train_MOG2_background_model(history=4, var_threshold=650, detect_shadows=False, frames=b, engine=eng) for b in bgs]
        frames = [b[0] for b in bgs]
        eng.set_grid(128, 128, 128)
        eng.set_cameras(fx.golden_cameras(), H, W)

        def device_path():
            eng.foreground_to_slot(models, frames, cam_bg_model_params, slot=0)
            eng.synchronize()
        res["foreground_to_slot_4cams_mog2_ms"] = _median_ms(device_path)
        for m in models:
            m.close()
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", help="also write the numbers as JSON to this file")
    main(ap.parse_args().out)
