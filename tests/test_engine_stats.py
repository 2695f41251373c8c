"""The stats dicts of CarveEngine's pass methods, key for key and type for type, without a device: the library is a fake
that fills every stats struct it is handed with a counting pattern, so a field that a method drops, renames or converts
differently shows as a changed dict.  The expected literals were taken from the hand-written conversions these methods had."""
import ctypes
import types

import numpy as np
import pytest

from voxcarve import _lib
from voxcarve.engine import DEFAULT_BOUNDS, CarveEngine


def _fill(st):
    """Field k gets k (k + 0.5 for a float); the elements of an array count on."""
    k = 0
    for name, ctype in st._fields_:
        if issubclass(ctype, ctypes.Array):
            arr = getattr(st, name)
            for i in range(len(arr)):
                arr[i] = k + i
            k += len(arr)
        else:
            setattr(st, name, k + 0.5 if ctype is ctypes.c_float else k)
            k += 1


class _FakeLib:
    def __getattr__(self, name):
        def call(*args):
            for a in args:
                obj = getattr(a, "_obj", None)               # what ctypes.byref() wraps
                if isinstance(obj, ctypes.Structure):
                    _fill(obj)
            return 0
        return call


@pytest.fixture
def eng():
    e = CarveEngine.__new__(CarveEngine)
    e._L, e._ctx = _FakeLib(), None
    e.grid, e.bounds, e.slab = (4, 4, 4), DEFAULT_BOUNDS, (0, 4)
    e.n_cameras, e.image_size, e.count = 2, (3, 5), 0
    return e


def _view():
    return types.SimpleNamespace(K=np.diag([100.0, 100.0, 1.0]), dist=np.zeros(5), R=np.eye(3), tvec=np.zeros(3))


def _same(got, want, where):
    assert type(got) is type(want), "%s: %s %r, expected %s %r" % (where, type(got).__name__, got, type(want).__name__, want)
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), "%s: keys %s, expected %s" % (where, sorted(got), sorted(want))
        for k in want:
            _same(got[k], want[k], "%s[%r]" % (where, k))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), "%s: %r, expected %r" % (where, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (where, i))
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and np.array_equal(got, want), "%s: %r, expected %r" % (where, got, want)
    else:
        assert got == want, "%s: %r, expected %r" % (where, got, want)


_MORPH = {"survivors_before": 0, "eroded": 1, "survivors_after": 2, "max_d2": 3, "q": (4, 5, 6), "morph_ms": 7.5}
_GROW = {"survivors_before": 0, "dilated": 1, "survivors_after": 2, "added": 3, "box_cells": 4, "q": (5, 6, 7), "grow_ms": 8.5}
_SETOP = {"survivors_before": 0, "other": 1, "common": 2, "survivors_after": 3, "added": 4, "removed": 5, "setop_ms": 6.5}
_COMPARE = {"a": 0, "b": 1, "common": 2, "only_a": 3, "only_b": 4, "diff_lo": (5, 6, 7), "diff_hi": (8, 9, 10), "compare_ms": 18.5,
            "iou": 2 / 9, "dice": 4.0, "hausdorff_mm": None}

# (method, arguments, the dict it returns, count afterwards (None: untouched), the size attributes it leaves)
CASES = [
    ("photo_carve", {}, {"rounds": 0, "converged": True, "survivors_before": 2, "survivors_after": 3, "photo_ms": 4.5},
     3, {"_photo_n": 2}),
    ("filter_components", {}, {"components": 0, "components_kept": 1, "survivors_before": 2, "survivors_after": 3, "largest": 4,
                               "components_ms": 5.5}, 3, {"_cc_n": 2, "_cc_k": 0}),
    ("hull_distance", {}, {"survivors": 0, "sites_inside_box": 1, "max_d2": 2, "q": (3, 4, 5), "distance_ms": 6.5}, None, {}),
    ("erode_hull", {"radius_mm": 1.0}, _MORPH, 2, {}),
    ("open_hull", {"radius_mm": 1.0}, _MORPH, 2, {}),
    ("dilate_hull", {"radius_mm": 1.0}, _GROW, 2, {}),
    ("close_hull", {"radius_mm": 1.0}, _GROW, 2, {}),
    ("temporal_filter", {"window": 3}, {"window": 0, "frames": 1, "on": 2, "off": 3, "survivors_before": 4, "survivors_after": 5,
                                        "added": 6, "removed": 7, "raw_changed": 8, "out_changed": 9, "temporal_ms": 10.5}, 5, {}),
    ("combine_hull", {"op": "and"}, _SETOP, 3, {}),
    ("compare_hull", {}, _COMPARE, None, {}),
    ("compare_hull", {"distance": True}, dict(_COMPARE, h2_ab=11, h2_ba=12, arg_ab=13, arg_ba=14, q=(15, 16, 17),
                                              hausdorff_mm=float(np.sqrt(12.0)) / 1000.0), None, {}),
    ("hull_normals", {"radius_mm": 1.0}, {"survivors": 0, "surface": 1, "zero": 2, "offsets": 3, "q": (4, 5, 6), "ext": (7, 8, 9),
                                          "normals_ms": 10.5}, None, {}),
    ("hull_geodesic", {}, {"survivors": 0, "seeds": 1, "reached": 2, "unreached": 3, "max_d": 4, "tile_visits": 5, "tiles": 6,
                           "edge_um": (7, 8, 9, 10, 11, 12, 13), "q": (14, 15, 16), "extremities": 17, "rounds": 18, "launches": 19,
                           "geodesic_ms": 20.5}, None, {"_geo_k": 17}),
    ("measure_hull", {}, {"survivors": 0, "groups": 3, "measured": 1, "unlabelled": 2, "measure_ms": 4.5}, None, {"_ms_g": 3}),
    ("hull_shell", {"level": 1}, {"survivors": 0, "cells_on": 1, "shell": 2, "faces": [3, 4, 5, 6, 7, 8], "level": 9, "cube_scale": 10,
                                  "dims": [11, 12, 13], "shell_ms": 14.5}, None, {"_shell_t": 2}),
    ("thin_hull", {}, {"survivors": 0, "anchors": 1, "kept": 2, "removed": 3, "isolated": 4, "endpoints": 5, "junctions": 6,
                       "passes": 7, "steps": 8, "launches": 9, "stable": 10, "thin_ms": 11.5}, None, {"_thin": (0, 2)}),
]


@pytest.mark.parametrize("method,kwargs,want,count,attrs", CASES, ids=["%s%s" % (c[0], "-distance" if c[1].get("distance") else "")
                                                                       for c in CASES])
def test_stats_dict(eng, method, kwargs, want, count, attrs):
    eng.count = 77
    _same(getattr(eng, method)(**kwargs), want, method)
    assert eng.count == (77 if count is None else count) and type(eng.count) is int
    for name, value in attrs.items():
        _same(getattr(eng, name), value, name)


def test_cluster_hull_adds_k_and_the_centres(eng):
    got = eng.cluster_hull(2)
    centres = np.array([[DEFAULT_BOUNDS[0], DEFAULT_BOUNDS[2]]] * 2)        # (the fetch that follows leaves its array zero)
    _same(got, {"survivors": 0, "columns": 1, "weight": 2, "iterations": 5, "converged": True, "q": (3, 4), "clusters_ms": 7.5,
                "k": 2, "centres_mm": centres}, "cluster_hull")
    assert eng._cl_k == 2 and eng.count == 0


def test_render_mesh_and_texture_nest_their_stats(eng):
    out = eng.render([_view(), _view()], 3, 5)
    _same(out["stats"], {"pixels": 0, "hits": 1, "cells_visited": 2, "blocks_skipped": 3, "render_ms": 4.5}, "render")
    assert list(out) == ["rgb", "depth", "index", "face", "stats"] and out["rgb"].shape == (2, 3, 5, 3)
    assert eng._render_shape == (2, (3, 5))
    tex = eng.texture_render()
    _same(tex["stats"], {"pixels": 0, "hits": 1, "refined": 2, "textured": 3, "fallback": 4, "point_tests": 5, "texture_ms": 6.5},
          "texture_render")
    assert list(tex) == ["rgb", "depth", "count", "best_cam", "refined", "stats"] and tex["refined"].shape == (2, 3, 5)
    mesh = eng.surface_mesh()
    _same(mesh["stats"], {"n_verts": 0, "n_faces": 1, "refined": 2, "unrefined": 3, "point_tests": 4, "surface_ms": 5.5}, "surface_mesh")
    assert list(mesh) == ["verts", "faces", "rgb", "refined", "stats"] and mesh["verts"].shape == (0, 3) and mesh["faces"].shape == (1, 3)
    assert eng._mesh_verts == 0


def test_every_stats_struct_is_covered():
    """A new Vc*Stats struct needs a case here."""
    covered = {"VcPhotoStats", "VcRenderStats", "VcComponentStats", "VcDistanceStats", "VcMorphStats", "VcGrowStats", "VcTemporalStats",
               "VcSetopStats", "VcCompareStats", "VcNormalsStats", "VcClusterStats", "VcGeodesicStats", "VcMeasureStats", "VcShellStats",
               "VcThinStats", "VcSurfaceStats", "VcTextureStats"}
    assert {n for n in dir(_lib) if n.startswith("Vc") and n.endswith("Stats")} == covered
