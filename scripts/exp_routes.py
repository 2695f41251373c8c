"""Synchronous carves over the route-kinds test's grids x option rows x modes x thresholds (tests/test_gpu_camera_counts.py): the
workload of the launch-trace comparison of two library builds (rocprofv3 --kernel-trace -- python scripts/exp_routes.py, the
library picked with VOXCARVE_LIB).  Prints the survivor counts' checksum."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fixtures_util as fx
import test_gpu_camera_counts as t
import voxcarve

C, cc, total = 4, 2, 0
cams, masks, frames = fx.random_scene(321, C=C, H=60, W=80, fg=0.55)
with voxcarve.CarveEngine(0) as eng:
    for grid in t.ROUTE_GRIDS:
        t.load(eng, grid, cams, masks, cc, frames[cc])
        for opts in t.ROUTE_ROWS:
            with t.Options(eng, opts):
                for mode in ("lut", "fused"):
                    for mv, vm in ((C, False), (C, True), (C - 1, False)):
                        total += eng.carve(mode=mode, min_views=mv, color_cam=cc, viewmask=vm)
print("survivors over all steps:", total)
