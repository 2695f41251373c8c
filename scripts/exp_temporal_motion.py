"""Cost of the motion-compensated vote (vc_hull_temporal_motion) against the same job done unfused with the calls
that were there before it: (a) 128^3, 512^3 and 1024^3 with the 4 real cameras and the committed MOG masks; (b) config 5, 512^3 x
16 ring cameras at 1080p.  Frame t is the carve of the masks with 2 % of the pixels flipped (tests/temporal_np.noisy_masks) and
rolled by 2 t columns.  Window 5, majority, motion 8 / 4 / 4.  Every frame runs, one after the other in the same process and on
the same hull H_t:
  fused     temporal_filter(5, motion=(8, 4, 4)) on one engine
  motion    hull_motion(0, 8, 4, 4) against H_{t-1} in register 0 (the field the fused call makes inside)
  warp      warp_hull(0, 1): one k_motion_warp over the grid; the unfused job needs window of them (window - 1 snapshots and P)
  plain     temporal_filter(5) on a second engine (the vote, the record merge and the hand-over both calls share)
unfused = motion + window x warp + plain.  Frames 0 .. 4 fill the rings and warm up; the REPS frames after them are timed by the
calls' own HIP events: medians with min and max.  Reported beside them: fused / unfused; align_vote_ms = fused - motion - plain,
what the aligning costs on top of a field and a plain vote (no kernel trace is taken here); and the traffic floor of the call,
m + 1 word streams read and m + 1 written at the 6.29 TB/s copy ceiling of DESIGN section 4, with its share of the fused time.
--reps N (default 9), --quick (128^3 and 512^3 only, 3 repetitions), --out FILE keeps the numbers as JSON.  Needs an MI355X."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW, PARAMS, STEP = 5, (8, 4, 4), 2
COPY_TBS = 6.29                                                  # the copy ceiling of DESIGN section 4


def _case(eng, eng2, grid, cameras, masks, reps):
    import temporal_np as tn
    case = {"grid": grid, "cameras": cameras, "window": WINDOW, "params": PARAMS, "step_columns": STEP}
    rows = {}
    eng.temporal_reset()
    eng2.temporal_reset()
    for t in range(WINDOW + reps):
        ms = [np.ascontiguousarray(np.roll(m, STEP * t, axis=1)) for m in tn.noisy_masks(masks, t)]
        eng.upload_masks(ms)
        eng.carve(mode="fused")
        eng2.upload_masks(ms)
        eng2.carve(mode="fused")
        got = {}
        if t:
            got["motion"] = eng.hull_motion(0, *PARAMS)["motion_ms"]
            got["warp"] = eng.warp_hull(0, 1)["warp_ms"]
        eng.keep_hull(0)
        st = eng.temporal_filter(WINDOW, motion=PARAMS)
        got["fused"] = st["temporal_ms"]
        got["plain"] = eng2.temporal_filter(WINDOW)["temporal_ms"]
        if t >= WINDOW:
            assert st["frames"] == WINDOW
            for k, v in got.items():
                rows.setdefault(k, []).append(v)
    case["stats"] = {k: v for k, v in st.items() if k != "temporal_ms"}
    for name, v in rows.items():
        a = np.array(v)
        case[name] = {"ms": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
    unfused = case["motion"]["ms"] + WINDOW * case["warp"]["ms"] + case["plain"]["ms"]
    nwords = (grid ** 3 + 63) // 64
    floor_ms = 2 * (WINDOW + 1) * nwords * 8 / (COPY_TBS * 1e12) * 1e3
    case.update(unfused_ms=unfused, fused_over_unfused=case["fused"]["ms"] / unfused, floor_ms=floor_ms,
                align_vote_ms=case["fused"]["ms"] - case["motion"]["ms"] - case["plain"]["ms"],
                floor_share_of_fused=floor_ms / case["fused"]["ms"])
    return case


def main():
    import fixtures_util as fx
    import voxcarve
    from voxcarve import synthetic
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 9
    quick = "--quick" in sys.argv
    if quick:
        reps = 3
    cams, masks = fx.golden_cameras(), fx.golden_masks()
    frames = fx.synthetic_frames(4, *masks[0].shape)
    H0, W0 = masks[0].shape
    res = {}
    with voxcarve.CarveEngine(0) as eng, voxcarve.CarveEngine(0) as eng2:
        for n in ((128, 512) if quick else (128, 512, 1024)):
            for e in (eng, eng2):
                e.set_grid(n, n, n)
                e.set_cameras(cams, H0, W0)
                e.upload_masks(masks)
                e.upload_frame(1, frames[1])
            res[str(n)] = _case(eng, eng2, n, 4, masks, reps)
            print(json.dumps(res[str(n)]), flush=True)
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            for e in (eng, eng2):
                e.set_grid(512, 512, 512)
                e.set_cameras(rc, H, W)
                e.upload_masks(rm)
            res["config5"] = _case(eng, eng2, 512, 16, rm, reps)
            print(json.dumps(res["config5"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
