"""ctypes binding of libvoxcarve.so (C ABI: include/voxcarve.h).

The library is the only compute path: if it is missing, or there is no gfx950
device, loading / context creation raises -- nothing here falls back to the CPU.
"""
import ctypes
import os

from . import lighting           # the lit pass's structs (vc_light_t, vc_light_stats_t) and its defaults
from . import motion             # the motion pass's structs (vc_motion_t, vc_motion_stats_t, vc_warp_stats_t, vc_temporal_motion_stats_t)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvoxcarve.so")

VC_OK = 0
VC_MODE_FUSED = 0
VC_MODE_LUT = 1
VC_FLAG_VIEWMASK = 1
VC_FLAG_NO_RECORDS = 2
VC_FOOT_ANY = 1
VC_FOOT_COVER = 2
VC_DIST_BORDER_OFF = 1
VC_DIST_OUTSIDE = 2
VC_MORPH_ERODE = 0
VC_MORPH_OPEN = 1
VC_GROW_DILATE = 0
VC_GROW_CLOSE = 1
VC_TEMPORAL_MAX_WINDOW = 15
VC_HULL_REGISTERS = 4
VC_SETOP_COPY, VC_SETOP_AND, VC_SETOP_OR, VC_SETOP_ANDNOT, VC_SETOP_XOR = 0, 1, 2, 3, 4
VC_COMPARE_DISTANCE = 1
VC_GEO_SEEDS_LIST, VC_GEO_SEEDS_IZ_MAX, VC_GEO_SEEDS_IZ_MIN = 0, 1, 2
VC_GEO_PATHS = 1
VC_GEO_MAX_K = 32
VC_GEO_TILE = (4, 64, 4)
VC_GEO_PAINT_LABELS, VC_GEO_PAINT_DISTANCE = 0, 1
VC_GEO_UNREACHED_RGB = (255, 0, 255)
VC_MEASURE_ALL, VC_MEASURE_CLUSTERS, VC_MEASURE_GEODESIC, VC_MEASURE_HOST = 0, 1, 2, 3
VC_MEASURE_PROFILE = 1
VC_MEASURE_MAX_GROUPS = 4096
VC_MEASURE_MAX_AXIS = 65536
VC_MEASURE_MAX_PROFILE = 1 << 20
VC_SHELL_MAX_LEVEL = 6
VC_THIN_CURVE, VC_THIN_POINT = 0, 1
VC_THIN_ANCHORS_NONE, VC_THIN_ANCHORS_LIST, VC_THIN_ANCHORS_EXTREMA = 0, 1, 2
VC_THIN_MAX_PASSES, VC_THIN_DEFAULT_PASSES = 10000, 4096
VC_THIN_TABLE_BYTES = 1 << 23
VC_MAX_CAMERAS = 16
VC_UNIQUE_ID_BYTES = 128
VC_MAX_MOG_MODELS = 64
VC_MOG2_MODEL_TAG = 0x10000

STATUS_NAMES = {0: "VC_OK", -1: "VC_ERR_ARG", -2: "VC_ERR_HIP", -3: "VC_ERR_RCCL",
                -4: "VC_ERR_OOM", -5: "VC_ERR_NODEV", -6: "VC_ERR_INTERNAL"}

c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_u16p = ctypes.POINTER(ctypes.c_uint16)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_i16p = ctypes.POINTER(ctypes.c_int16)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_f64p = ctypes.POINTER(ctypes.c_double)
c_ctx = ctypes.c_void_p


VC_KERNEL_KINDS, VC_WORK_KINDS = 28, 10
KERNEL_KINDS = ("k_prep_pack", "k_prep_grid", "k_cull_bricks", "k_brick_words", "k_voxel_words", "k_assemble", "k_scan_groups",
                "k_finish_scan", "k_emit", "one_launch_carve", "k_cull", "k_count_groups", "foot_table", "k_carve_foot",
                "k_dist_box", "k_dist_y", "k_dist_env", "k_dist_records", "geo_seed", "k_geo_tiles", "k_geo_sweep", "geo_argmax",
                "k_temporal_vote", "temporal_rank", "temporal_merge", "k_grow_mark", "grow_rank", "grow_merge")
WORK_KINDS = ("word_boxes", "table_entries", "projections", "emit_projections", "brick_boxes", "foot_projections", "foot_union_skips",
              "foot_words", "dist_cells", "dist_lines")


class VcTiming(ctypes.Structure):
    _fields_ = [("carve_ms", ctypes.c_float), ("compact_ms", ctypes.c_float),
                ("gather_ms", ctypes.c_float), ("lut_ms", ctypes.c_float),
                ("h2d_ms", ctypes.c_float), ("voxels", ctypes.c_uint64),
                ("survivors", ctypes.c_uint64), ("carve_launches", ctypes.c_uint32),
                ("carve_ms_sum", ctypes.c_float), ("first_ms", ctypes.c_float),
                ("first_ms_sum", ctypes.c_float), ("exchange_ms", ctypes.c_float),
                ("gather_ms_sum", ctypes.c_float), ("gathers", ctypes.c_uint32),
                ("prep_ms", ctypes.c_float), ("prep_ms_sum", ctypes.c_float), ("preps", ctypes.c_uint32),
                ("preps_timed", ctypes.c_uint32), ("emit_ms", ctypes.c_float), ("emit_ms_sum", ctypes.c_float),
                ("emit_launches", ctypes.c_uint32),
                ("kernel_ms_sum", ctypes.c_float * VC_KERNEL_KINDS), ("kernel_launches", ctypes.c_uint32 * VC_KERNEL_KINDS),
                ("work", ctypes.c_uint64 * VC_WORK_KINDS), ("visible_ms", ctypes.c_float), ("thin_ms", ctypes.c_float),
                ("thin_kernel_ms", ctypes.c_float), ("thin_launches", ctypes.c_uint32)]


class VcPhotoStats(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_uint32), ("converged", ctypes.c_uint32), ("survivors_before", ctypes.c_uint64),
                ("survivors_after", ctypes.c_uint64), ("photo_ms", ctypes.c_float)]


class VcView(ctypes.Structure):
    _fields_ = [("K", ctypes.c_double * 4), ("dist", ctypes.c_double * 5), ("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3)]


class VcRenderStats(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("cells_visited", ctypes.c_uint64),
                ("blocks_skipped", ctypes.c_uint64), ("render_ms", ctypes.c_float)]


class VcComponentStats(ctypes.Structure):
    _fields_ = [("components", ctypes.c_uint32), ("components_kept", ctypes.c_uint32), ("survivors_before", ctypes.c_uint64),
                ("survivors_after", ctypes.c_uint64), ("largest", ctypes.c_uint32), ("components_ms", ctypes.c_float)]


class VcDistanceStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("sites_inside_box", ctypes.c_uint64), ("max_d2", ctypes.c_uint64),
                ("q", ctypes.c_uint64 * 3), ("distance_ms", ctypes.c_float)]


class VcMorphStats(ctypes.Structure):
    _fields_ = [("survivors_before", ctypes.c_uint64), ("eroded", ctypes.c_uint64), ("survivors_after", ctypes.c_uint64),
                ("max_d2", ctypes.c_uint64), ("q", ctypes.c_uint64 * 3), ("morph_ms", ctypes.c_float)]


class VcGrowStats(ctypes.Structure):
    _fields_ = [("survivors_before", ctypes.c_uint64), ("dilated", ctypes.c_uint64), ("survivors_after", ctypes.c_uint64),
                ("added", ctypes.c_uint64), ("box_cells", ctypes.c_uint64), ("q", ctypes.c_uint64 * 3), ("grow_ms", ctypes.c_float)]


class VcTemporalStats(ctypes.Structure):
    _fields_ = [("window", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("on", ctypes.c_uint32), ("off", ctypes.c_uint32),
                ("survivors_before", ctypes.c_uint64), ("survivors_after", ctypes.c_uint64), ("added", ctypes.c_uint64),
                ("removed", ctypes.c_uint64), ("raw_changed", ctypes.c_uint64), ("out_changed", ctypes.c_uint64),
                ("temporal_ms", ctypes.c_float)]


class VcSetopStats(ctypes.Structure):
    _fields_ = [("survivors_before", ctypes.c_uint64), ("other", ctypes.c_uint64), ("common", ctypes.c_uint64),
                ("survivors_after", ctypes.c_uint64), ("added", ctypes.c_uint64), ("removed", ctypes.c_uint64), ("setop_ms", ctypes.c_float)]


class VcCompareStats(ctypes.Structure):
    _fields_ = [("a", ctypes.c_uint64), ("b", ctypes.c_uint64), ("common", ctypes.c_uint64), ("only_a", ctypes.c_uint64),
                ("only_b", ctypes.c_uint64), ("diff_lo", ctypes.c_uint32 * 3), ("diff_hi", ctypes.c_uint32 * 3),
                ("h2_ab", ctypes.c_uint64), ("h2_ba", ctypes.c_uint64), ("arg_ab", ctypes.c_uint32), ("arg_ba", ctypes.c_uint32),
                ("q", ctypes.c_uint64 * 3), ("compare_ms", ctypes.c_float)]


class VcNormalsStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("surface", ctypes.c_uint64), ("zero", ctypes.c_uint64), ("offsets", ctypes.c_uint64),
                ("q", ctypes.c_uint64 * 3), ("ext", ctypes.c_uint32 * 3), ("normals_ms", ctypes.c_float)]


class VcCluster(ctypes.Structure):
    _fields_ = [("centre_um", ctypes.c_int64 * 2), ("voxels", ctypes.c_uint64), ("weight", ctypes.c_uint64),
                ("columns", ctypes.c_uint32), ("lo", ctypes.c_uint32 * 3), ("hi", ctypes.c_uint32 * 3)]


class VcClusterStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("columns", ctypes.c_uint64), ("weight", ctypes.c_uint64), ("q", ctypes.c_uint64 * 2),
                ("iterations", ctypes.c_uint32), ("converged", ctypes.c_uint32), ("clusters_ms", ctypes.c_float)]


class VcExtremum(ctypes.Structure):
    _fields_ = [("d", ctypes.c_uint64), ("voxel", ctypes.c_uint32), ("record", ctypes.c_uint32), ("ix", ctypes.c_uint32),
                ("iy", ctypes.c_uint32), ("iz", ctypes.c_uint32), ("label", ctypes.c_uint32)]


class VcGeodesicStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("seeds", ctypes.c_uint64), ("reached", ctypes.c_uint64), ("unreached", ctypes.c_uint64),
                ("max_d", ctypes.c_uint64), ("tile_visits", ctypes.c_uint64), ("tiles", ctypes.c_uint64), ("edge_um", ctypes.c_uint64 * 7),
                ("q", ctypes.c_uint64 * 3), ("extremities", ctypes.c_uint32), ("rounds", ctypes.c_uint32), ("launches", ctypes.c_uint32),
                ("geodesic_ms", ctypes.c_float)]


class VcMeasure(ctypes.Structure):
    _fields_ = [("voxels", ctypes.c_uint64), ("surface", ctypes.c_uint64), ("seen", ctypes.c_uint64), ("s1", ctypes.c_uint64 * 3),
                ("s2", ctypes.c_uint64 * 6), ("faces", ctypes.c_uint64 * 6), ("rgb", ctypes.c_uint64 * 3), ("lo", ctypes.c_uint32 * 3),
                ("hi", ctypes.c_uint32 * 3)]


class VcMeasureStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("measured", ctypes.c_uint64), ("unlabelled", ctypes.c_uint64),
                ("groups", ctypes.c_uint32), ("measure_ms", ctypes.c_float)]


class VcShellStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("cells_on", ctypes.c_uint64), ("shell", ctypes.c_uint64), ("faces", ctypes.c_uint64 * 6),
                ("level", ctypes.c_uint32), ("cube_scale", ctypes.c_uint32), ("dims", ctypes.c_uint32 * 3), ("shell_ms", ctypes.c_float)]


class VcSkeletonVoxel(ctypes.Structure):
    _fields_ = [("voxel", ctypes.c_uint32), ("record", ctypes.c_uint32), ("degree", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 3)]


class VcThinStats(ctypes.Structure):
    _fields_ = [("survivors", ctypes.c_uint64), ("anchors", ctypes.c_uint64), ("kept", ctypes.c_uint64), ("removed", ctypes.c_uint64),
                ("isolated", ctypes.c_uint64), ("endpoints", ctypes.c_uint64), ("junctions", ctypes.c_uint64),
                ("passes", ctypes.c_uint32), ("steps", ctypes.c_uint32), ("launches", ctypes.c_uint32), ("stable", ctypes.c_uint32),
                ("thin_ms", ctypes.c_float)]


class VcSurfaceStats(ctypes.Structure):
    _fields_ = [("n_verts", ctypes.c_uint64), ("n_faces", ctypes.c_uint64), ("refined", ctypes.c_uint64),
                ("unrefined", ctypes.c_uint64), ("point_tests", ctypes.c_uint64), ("surface_ms", ctypes.c_float)]


class VcTextureStats(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_uint64), ("hits", ctypes.c_uint64), ("refined", ctypes.c_uint64), ("textured", ctypes.c_uint64),
                ("fallback", ctypes.c_uint64), ("point_tests", ctypes.c_uint64), ("texture_ms", ctypes.c_float)]


class VcComponent(ctypes.Structure):
    _fields_ = [("label", ctypes.c_uint32), ("size", ctypes.c_uint32), ("lo", ctypes.c_uint32 * 3), ("hi", ctypes.c_uint32 * 3),
                ("kept", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


# name -> (restype, argtypes); every symbol include/voxcarve.h declares.
SIGNATURES = {
    "vc_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "vc_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_ctx)]),
    "vc_destroy": (ctypes.c_int, [c_ctx]),
    "vc_last_error": (ctypes.c_char_p, [c_ctx]),
    "vc_synchronize": (ctypes.c_int, [c_ctx]),
    "vc_set_grid": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, c_f64p]),
    "vc_set_slab": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32]),
    "vc_get_axes": (ctypes.c_int, [c_ctx, c_f64p, c_f64p, c_f64p]),
    "vc_set_cameras": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_f64p, c_f64p, c_f64p, c_f64p,
                                      ctypes.c_uint32, ctypes.c_uint32]),
    "vc_upload_masks": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p]),
    "vc_touch_masks": (ctypes.c_int, [c_ctx, ctypes.c_uint32]),
    "vc_set_mask_postfilter": (ctypes.c_int, [c_ctx, c_u8p, c_u8p]),
    "vc_fetch_mask": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, c_u8p]),
    "vc_bgr_to_hsv": (ctypes.c_int, [c_ctx, c_u8p, ctypes.c_uint32, ctypes.c_uint32, c_u8p]),
    "vc_mask_morphology": (ctypes.c_int, [c_ctx, c_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, c_u8p]),
    "vc_mog_create": (ctypes.c_int, [c_ctx, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_uint32)]),
    "vc_mog_apply": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, c_u8p]),
    "vc_mog_state": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32),
                                    ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "vc_mog_destroy": (ctypes.c_int, [c_ctx, ctypes.c_uint32]),
    "vc_mog2_create": (ctypes.c_int, [c_ctx, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double,
                                      ctypes.POINTER(ctypes.c_uint32)]),
    "vc_mog2_apply": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, c_u8p]),
    "vc_mog2_state": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.c_uint64, c_u8p, ctypes.c_uint64,
                                     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                     ctypes.POINTER(ctypes.c_uint32)]),
    "vc_mog2_destroy": (ctypes.c_int, [c_ctx, ctypes.c_uint32]),
    "vc_foreground_front": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_double,
                                           ctypes.c_int, ctypes.c_int, c_u8p]),
    "vc_fill_figures": (ctypes.c_int, [c_ctx, c_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, c_u8p]),
    "vc_foreground_to_slot": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u32p, ctypes.c_uint32, c_u8p, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_double, c_f64p, c_f64p, c_u8p, c_u8p]),
    "vc_upload_frame": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, c_u8p]),
    "vc_build_lut": (ctypes.c_int, [c_ctx]),
    "vc_fetch_lut": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_i32p]),
    "vc_upload_lut": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_i32p]),
    "vc_project": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_f64p, ctypes.c_uint64, c_f64p]),
    "vc_carve": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                ctypes.c_uint32, c_u64p]),
    "vc_carve_footprint": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, c_u64p]),
    "vc_carve_begin": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]),
    "vc_carve_end": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_fetch": (ctypes.c_int, [c_ctx, c_u32p, c_u8p, c_u8p]),
    "vc_fetch_records": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_host_alloc": (ctypes.c_int, [c_ctx, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]),
    "vc_host_free": (ctypes.c_int, [c_ctx, ctypes.c_void_p]),
    "vc_fetch_viewmask": (ctypes.c_int, [c_ctx, c_u16p]),
    "vc_fetch_occupancy": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_color_visible": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32]),
    "vc_fetch_visibility": (ctypes.c_int, [c_ctx, c_u16p]),
    "vc_fetch_depth": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]),
    "vc_photo_carve": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.POINTER(VcPhotoStats)]),
    "vc_fetch_photo_rounds": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_hull_components": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.POINTER(VcComponentStats)]),
    "vc_fetch_component_labels": (ctypes.c_int, [c_ctx, c_u32p]),
    "vc_fetch_components": (ctypes.c_int, [c_ctx, ctypes.c_void_p]),
    "vc_render": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, c_u8p, c_u8p,
                                 ctypes.c_uint32, ctypes.c_void_p]),
    "vc_fetch_render": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u32p, ctypes.POINTER(ctypes.c_float), c_u8p, c_u8p]),
    "vc_marching_cubes": (ctypes.c_int, [c_ctx, c_u8p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, c_u64p, c_u64p]),
    "vc_fetch_mesh": (ctypes.c_int, [c_ctx, ctypes.POINTER(ctypes.c_float), c_u32p]),
    "vc_surface_mesh": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VcSurfaceStats)]),
    "vc_fetch_surface_mesh": (ctypes.c_int, [c_ctx, c_f64p, c_u32p, c_u8p, c_u8p]),
    "vc_hull_distance": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.POINTER(VcDistanceStats)]),
    "vc_fetch_record_distance": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_fetch_distance": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u64p]),
    "vc_hull_morphology": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(VcMorphStats)]),
    "vc_hull_grow": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(VcGrowStats)]),
    "vc_fetch_grown": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_hull_temporal": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.POINTER(VcTemporalStats)]),
    "vc_fetch_temporal": (ctypes.c_int, [c_ctx, c_u8p, c_u8p]),
    "vc_fetch_temporal_history": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p]),
    "vc_temporal_reset": (ctypes.c_int, [c_ctx]),
    "vc_hull_keep": (ctypes.c_int, [c_ctx, ctypes.c_uint32]),
    "vc_hull_upload": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, c_u64p, ctypes.c_uint64]),
    "vc_hull_release": (ctypes.c_int, [c_ctx, ctypes.c_uint32]),
    "vc_fetch_kept": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, c_u64p, c_u64p, c_u32p]),
    "vc_hull_combine": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VcSetopStats)]),
    "vc_fetch_combined": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_hull_compare": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VcCompareStats)]),
    "vc_hull_motion": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.POINTER(motion.MotionStats)]),
    "vc_fetch_motion": (ctypes.c_int, [c_ctx, ctypes.c_void_p, c_u64p]),
    "vc_hull_warp": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(motion.WarpStats)]),
    "vc_paint_motion": (ctypes.c_int, [c_ctx]),
    "vc_hull_motion_pyramid": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(motion.PyramidStats)]),
    "vc_fetch_motion_level": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_void_p, c_u64p]),
    "vc_fetch_motion_occupancy": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, c_u64p, c_u64p]),
    "vc_hull_temporal_motion": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(motion.TemporalMotionStats)]),
    "vc_fetch_temporal_motion": (ctypes.c_int, [c_ctx, ctypes.c_void_p, c_u64p]),
    "vc_hull_normals": (ctypes.c_int, [c_ctx, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(VcNormalsStats)]),
    "vc_fetch_record_normals": (ctypes.c_int, [c_ctx, c_i16p]),
    "vc_shade_render": (ctypes.c_int, [c_ctx, c_f64p, ctypes.c_uint32, ctypes.c_uint32]),
    "vc_fetch_shaded": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p]),
    "vc_surface_normals": (ctypes.c_int, [c_ctx, c_i16p]),
    "vc_texture_render": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_float, ctypes.c_uint32,
                                         ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VcTextureStats)]),
    "vc_fetch_textured": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, ctypes.POINTER(ctypes.c_float), c_u8p, c_u8p, c_u8p]),
    "vc_light_render": (ctypes.c_int, [c_ctx, ctypes.POINTER(lighting.Light), ctypes.c_uint32, ctypes.POINTER(lighting.LightStats)]),
    "vc_fetch_lit": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p, ctypes.POINTER(ctypes.c_float), c_u8p, c_u8p, c_u8p]),
    "vc_hull_clusters": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                        c_i64p, ctypes.c_uint32, ctypes.POINTER(VcClusterStats)]),
    "vc_fetch_cluster_labels": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_fetch_clusters": (ctypes.c_int, [c_ctx, ctypes.POINTER(VcCluster)]),
    "vc_fetch_cluster_histograms": (ctypes.c_int, [c_ctx, c_u32p]),
    "vc_fetch_floor_map": (ctypes.c_int, [c_ctx, c_u32p]),
    "vc_fetch_floor_labels": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_paint_clusters": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_hull_geodesic": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, c_u32p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint32, ctypes.POINTER(VcGeodesicStats)]),
    "vc_fetch_geodesic": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_fetch_geodesic_labels": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_fetch_extrema": (ctypes.c_int, [c_ctx, ctypes.POINTER(VcExtremum)]),
    "vc_geodesic_path": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u32p, ctypes.c_uint32, c_u32p]),
    "vc_fetch_extremum_path": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u32p, ctypes.c_uint32, c_u32p]),
    "vc_paint_geodesic": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u8p]),
    "vc_hull_measure": (ctypes.c_int, [c_ctx, ctypes.c_uint32, c_u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VcMeasureStats)]),
    "vc_fetch_measure": (ctypes.c_int, [c_ctx, ctypes.POINTER(VcMeasure)]),
    "vc_fetch_measure_profile": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_hull_shell": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(VcShellStats)]),
    "vc_fetch_shell": (ctypes.c_int, [c_ctx, c_u64p, c_u8p]),
    "vc_fetch_shell_viewer": (ctypes.c_int, [c_ctx, ctypes.c_double, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
    "vc_hull_thin": (ctypes.c_int, [c_ctx, ctypes.c_uint32, ctypes.c_uint32, c_u32p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.POINTER(VcThinStats)]),
    "vc_fetch_thin": (ctypes.c_int, [c_ctx, ctypes.POINTER(ctypes.c_uint16)]),
    "vc_fetch_skeleton": (ctypes.c_int, [c_ctx, ctypes.POINTER(VcSkeletonVoxel)]),
    "vc_fetch_thin_table": (ctypes.c_int, [c_ctx, c_u8p]),
    "vc_set_option": (ctypes.c_int, [c_ctx, ctypes.c_char_p, ctypes.c_int]),
    "vc_timing_struct_size": (ctypes.c_uint32, []),
    "vc_timing": (ctypes.c_int, [c_ctx, ctypes.POINTER(VcTiming)]),
    "vc_debug_counters": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_timing_reset": (ctypes.c_int, [c_ctx]),
    "vc_comm_unique_id": (ctypes.c_int, [c_u8p]),
    "vc_comm_init": (ctypes.c_int, [c_ctx, ctypes.c_int, ctypes.c_int, c_u8p]),
    "vc_comm_destroy": (ctypes.c_int, [c_ctx]),
    "vc_allgather": (ctypes.c_int, [c_ctx, c_u64p, c_u64p]),
    "vc_fetch_gathered": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_pack_entries": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_fetch_entries": (ctypes.c_int, [c_ctx, c_u64p]),
    "vc_expand_entries": (ctypes.c_int, [c_ctx, c_u64p, ctypes.c_uint64, c_u64p]),
    "vc_comm_allreduce_max": (ctypes.c_int, [c_ctx, c_f64p]),
}

_lib = None


class VoxcarveError(RuntimeError):
    pass


def load():
    """Load libvoxcarve.so and bind every entry point; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("VOXCARVE_LIB", LIB_PATH)          # an alternative build of the same library (sanitizer runs)
    if not os.path.exists(path):
        raise VoxcarveError(
            "libvoxcarve.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    # multi-process GPU work on this platform needs dmabuf IPC (RCCL's hipIpcGetMemHandle fails otherwise);
    # must be in the environment before the HIP runtime initialises
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = ABI drift, let it surface
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.vc_timing_struct_size() != ctypes.sizeof(VcTiming):
        raise VoxcarveError("libvoxcarve.so at %s was built with a vc_timing_t of %d bytes, this binding mirrors one of %d: rebuild the library"
                            % (path, lib.vc_timing_struct_size(), ctypes.sizeof(VcTiming)))
    _lib = lib
    return lib


def check(rc, ctx=None, what=""):
    if rc == VC_OK:
        return
    msg = load().vc_last_error(ctx)
    raise VoxcarveError("%s failed: %s (%s)" % (what or "voxcarve call", STATUS_NAMES.get(rc, rc),
                                                msg.decode() if msg else ""))
