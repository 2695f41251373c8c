"""Cost of the set algebra on hulls (vc_hull_combine, vc_hull_compare): (a) 128^3, 512^3 and 1024^3 with the 4 real
cameras and the committed MOG masks; (b) config 5, 512^3 x 16 ring cameras at 1080p.  A is the hull of the masks as they are, B
the hull of the masks with the seeded noise of the temporal recipe (2 % of each mask's pixels flipped, generator 7001); B sits in
register 0 with its records (keep_hull) and in register 1 as bits only (upload_hull).  Every repetition carves A again and runs, one
after the other in the same process:
  yardstick    vc_hull_temporal(window 2, keep_on 1, keep_off 1) on A with B as the ring's older hull: O = A | B, the same set as
               combine "or", one more word array read, the same record merge, fresh records coloured from the colour camera
  or_bits      combine_hull("or", 1): fresh records coloured as the yardstick's
  or_records   combine_hull("or", 0): the added voxels take B's records
  andnot, and, xor, copy   against register 0
  compare      compare_hull(0)                  beside  vc_hull_measure("all")
  compare_d    compare_hull(0, distance=True)   beside  two vc_hull_distance calls (inside field over the hull's box)
Times are the calls' own HIP events (setop_ms, temporal_ms, compare_ms, ...), medians with min and max of the repetitions after a
warm-up round.  --reps N (default 9), --quick (1024^3 only, 3 repetitions: a profiler run), --out FILE keeps the numbers as JSON.
Needs an MI355X."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOISE = 0.02


def _noisy(masks, t):
    rng = np.random.default_rng(7000 + t)
    return [np.where(rng.random(m.shape) < NOISE, 255 - m, m).astype(np.uint8) for m in masks]


def _case(eng, grid, cameras, masks, other, reps):
    nwords = (grid ** 3 + 63) // 64
    case = {"grid": grid, "cameras": cameras, "nwords": nwords, "or_words_bytes": 3 * nwords * 8}

    def carve(m):
        eng.upload_masks(m)
        return eng.carve(mode="fused")

    carve(other)
    eng.keep_hull(0)
    raw = np.empty(nwords, dtype=np.uint64)                        # (the words as they are: no bool volume of 2^30 elements on the host)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    eng._check(eng._L.vc_fetch_occupancy(eng._ctx, raw.ctypes.data_as(u8)), "vc_fetch_occupancy")
    eng._check(eng._L.vc_hull_upload(eng._ctx, 1, raw.ctypes.data_as(u8), None, 0), "vc_hull_upload")
    case["survivors_b"] = eng.count
    rows = {}

    def note(name, ms):
        rows.setdefault(name, []).append(ms)

    for rep in range(reps + 1):                                    # round 0 allocates and warms up
        eng.temporal_reset()
        carve(other)
        eng.temporal_filter(2, 1, 1)
        carve(masks)
        st = eng.temporal_filter(2, 1, 1)
        yard = st
        for name, op, reg in (("or_bits", "or", 1), ("or_records", "or", 0), ("andnot", "andnot", 0), ("and", "and", 0), ("xor", "xor", 0),
                              ("copy", "copy", 0)):
            carve(masks)
            st = eng.combine_hull(op, reg)
            if rep:
                note(name, st["setop_ms"])
            case.setdefault("stats", {})[name] = {k: v for k, v in st.items() if k != "setop_ms"}
        if rep:
            note("yardstick", yard["temporal_ms"])
        carve(masks)
        cmp_ = eng.compare_hull(0)
        ms = eng.measure_hull("all")
        cmpd = eng.compare_hull(0, distance=True)
        d1 = eng.hull_distance()
        d2 = eng.hull_distance()
        if rep:
            note("compare", cmp_["compare_ms"])
            note("measure_all", ms["measure_ms"])
            note("compare_d", cmpd["compare_ms"])
            note("two_distance", d1["distance_ms"] + d2["distance_ms"])
    case["survivors_a"] = cmp_["a"]
    case["yardstick_stats"] = {k: v for k, v in yard.items() if k != "temporal_ms"}
    case["compare_stats"] = {k: v for k, v in cmpd.items() if k != "compare_ms"}
    for name, v in rows.items():
        a = np.array(v)
        case[name] = {"ms": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
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
    other = _noisy(masks, 1)
    res = {}
    with voxcarve.CarveEngine(0) as eng:
        for n in ((1024,) if quick else (128, 512, 1024)):
            eng.set_grid(n, n, n)
            eng.set_cameras(cams, H0, W0)
            eng.upload_masks(masks)
            eng.upload_frame(1, frames[1])
            res[str(n)] = _case(eng, n, 4, masks, other, reps)
            print(json.dumps(res[str(n)]), flush=True)
        if not quick:
            H, W = 1080, 1920
            rc = synthetic.ring_cameras(16, H, W)
            rm = synthetic.ellipsoid_masks(rc, H, W)
            eng.set_grid(512, 512, 512)
            eng.set_cameras(rc, H, W)
            eng.upload_masks(rm)
            res["config5"] = _case(eng, 512, 16, rm, _noisy(rm, 1), reps)
            print(json.dumps(res["config5"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
