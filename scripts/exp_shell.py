"""Cost of listing the hull's shell (vc_hull_shell) after a carve: (a) 128^3, 512^3 and 1024^3 with the 4 real
cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  Per case, on the carve's result
(mode="fused", min_views = all cameras): shell_ms (HIP events around the whole call, the count's read-back included) and the
host's wall clock at levels 0, 1 and 2, medians of the repetitions after a warm-up call, with the shell's size and its share of
the survivors.  The yardsticks, in the same run on the same hull: vc_hull_measure over the whole hull (measure_ms: it reads the
same records and the same six neighbour bits and writes nothing) and vc_hull_components with nothing removed (components_ms);
both are code this pass does not touch.
End to end, copies included, as wall clock on the host: hull_shell(0) + fetch_shell_viewer() -- the viewer's arrays of what can
be seen, made on the device -- against what the drop-in layer does without it: fetch() + voxel_keys + viewer_positions +
viewer_colors over every survivor in numpy.
--reps N (default 11; the end-to-end paths run max(N // 3, 1) times), --quick (1024^3 only, 3 repetitions: a profiler run),
--out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _shell(eng, reps, level):
    rows = []
    for _ in range(reps + 1):                                      # the first call allocates: left out
        t0 = time.perf_counter()
        st = eng.hull_shell(level)
        rows.append((st["shell_ms"], (time.perf_counter() - t0) * 1e3))
    a = np.array(rows[1:])
    return {"ms": float(np.median(a[:, 0])), "ms_min": float(a[:, 0].min()), "wall_ms": float(np.median(a[:, 1])),
            "cells_on": st["cells_on"], "shell": st["shell"], "faces": st["faces"], "dims": st["dims"],
            "share": st["shell"] / max(st["survivors"], 1)}


def _measure(eng, reps):
    dev = [eng.measure_hull()["measure_ms"] for _ in range(reps + 1)]
    return {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}


def _components(eng, reps):
    dev = [eng.filter_components()["components_ms"] for _ in range(reps + 1)]      # min_voxels = 0: labels, removes nothing
    return {"ms": float(np.median(dev[1:])), "ms_min": float(np.min(dev[1:]))}


def _end_to_end(eng, reps):
    from voxcarve.engine import viewer_colors, viewer_positions, voxel_keys
    shell, full = [], []
    rows = bytes_shell = 0
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        eng.hull_shell(0)
        pos, col = eng.fetch_shell_viewer()
        shell.append((time.perf_counter() - t0) * 1e3)
        rows, bytes_shell = len(pos), pos.nbytes + col.nbytes
        del pos, col
        t0 = time.perf_counter()
        idx, rgb, _ = eng.fetch()
        keys = voxel_keys(idx, eng.grid, eng.axes())
        pos, col = viewer_positions(keys), viewer_colors(rgb)
        full.append((time.perf_counter() - t0) * 1e3)
        n_full = len(pos)
        del idx, rgb, keys, pos, col
    return {"shell_wall_ms": float(np.median(shell[1:])), "full_wall_ms": float(np.median(full[1:])), "shell_rows": rows,
            "full_rows": n_full, "shell_bytes_copied": bytes_shell, "full_bytes_copied": 8 * n_full,
            "full_over_shell": float(np.median(full[1:]) / np.median(shell[1:]))}


def _case(eng, grid, cameras, reps):
    S = eng.carve(mode="fused")
    case = {"grid": grid, "cameras": cameras, "survivors": S}
    for level in (0, 1, 2):
        case["level%d" % level] = _shell(eng, reps, level)
    case["hull_measure"] = _measure(eng, reps)
    case["hull_components"] = _components(eng, reps)
    for level in (0, 1, 2):
        case["level%d_over_hull_measure" % level] = case["level%d" % level]["ms"] / case["hull_measure"]["ms"]
        case["level%d_over_hull_components" % level] = case["level%d" % level]["ms"] / case["hull_components"]["ms"]
    case["end_to_end"] = _end_to_end(eng, max(reps // 3, 1))
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
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
