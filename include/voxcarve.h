/* voxcarve.h -- C ABI of libvoxcarve.so, the MI355X (gfx950) visual-hull carve engine.
 *
 * Drop-in boundary for ONE path of ChristosP1/Voxel-Based-3D-Reconstruction: the
 * per-voxel x per-camera projection-and-mask test behind set_voxel_positions().
 * The reference is pure Python; a maintainer binds this library with ctypes (stub in
 * INTEGRATION.md).  Each entry point names the reference interface it replaces
 * (paths relative to the reference root).
 *
 * Conventions: every function returns 0 (VC_OK) or a negative vc_status; the message
 * of the last failure is vc_last_error(ctx).  A context owns one HIP device + stream
 * and all device buffers; it is NOT thread-safe (the reference calls the path from one
 * thread, executable.py:182-188).  Host buffers belong to the caller.  An empty
 * result is count 0, not an error (reference returns [], []).
 *
 * Voxel numbering (voxel_reconstruction.py:52-57): linear index
 *     i = iz*nx*ny + ix*ny + iy,   centre = (xs[ix], ys[iy], zs[iz]),
 * axes = np.linspace(lo, hi, n).  Survivor lists are ascending in i, which is the
 * order the reference's dicts yield (assignment.py:121-133).
 */
#ifndef VOXCARVE_H
#define VOXCARVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vc_ctx vc_ctx;

typedef enum {
    VC_OK = 0,
    VC_ERR_ARG = -1,    /* bad argument / call order */
    VC_ERR_HIP = -2,    /* HIP runtime error (message has hipGetErrorString) */
    VC_ERR_RCCL = -3,   /* RCCL missing or failed */
    VC_ERR_OOM = -4,    /* device allocation failed */
    VC_ERR_NODEV = -5,  /* no usable GPU: there is NO CPU fallback */
    VC_ERR_INTERNAL = -6 /* a bound the library sets for itself was exceeded (vc_hull_geodesic's rounds) */
} vc_status;

typedef enum {
    VC_MODE_FUSED = 0,  /* project in-kernel (fp64), nothing precomputed            */
    VC_MODE_LUT = 1     /* stream the packed int32 LUT built by vc_build_lut()      */
} vc_mode;

enum {
    VC_FOOT_ANY = 1u,        /* vc_carve_footprint: a camera passes when any pixel of the voxel's box is foreground   */
    VC_FOOT_COVER = 2u       /* ... when at least q / 256 of the box is (q = 256: the whole box, inside the image)     */
};

enum {
    VC_FLAG_VIEWMASK = 1u,   /* also keep the per-voxel camera bitmask (compat dicts) */
    VC_FLAG_NO_RECORDS = 2u  /* count + occupancy only: the records are produced by vc_allgather /
                                vc_expand_entries (a rank of a multi-GPU job never reads its own slab's list).
                                With a communicator attached (vc_comm_init) such a step is a COLLECTIVE call:
                                it also packs the slab's words and all-gathers the counts, so every rank
                                must issue the same sequence of them. */
};

#define VC_MAX_CAMERAS 16
#define VC_UNIQUE_ID_BYTES 128

typedef enum {
    VC_K_PREP_PACK = 0, VC_K_PREP_GRID, VC_K_CULL_BRICKS, VC_K_BRICK_WORDS, VC_K_VOXEL_WORDS, VC_K_ASSEMBLE,
    VC_K_SCAN_GROUPS, VC_K_FINISH_SCAN, VC_K_EMIT, VC_K_CARVE_ONE_LAUNCH /* k_lut_refine, k_carve_fused*, k_carve_generic, k_lut_first */,
    VC_K_CULL /* in front of a one-launch kernel */, VC_K_COUNT_GROUPS,
    VC_K_FOOT_TABLE /* k_foot_rows + k_foot_cols */, VC_K_FOOT_CARVE /* k_carve_foot */,
    VC_K_DIST_BOX /* k_dist_box */, VC_K_DIST_Y /* k_dist_y */, VC_K_DIST_ENV /* k_dist_env, along x and along z */,
    VC_K_DIST_RECORDS /* k_dist_records */,
    VC_K_GEO_SEED /* k_geo_seed_list, k_geo_seed_layers, k_geo_source */, VC_K_GEO_TILES /* k_geo_tiles */,
    VC_K_GEO_SWEEP /* k_geo_sweep */, VC_K_GEO_ARGMAX /* k_geo_best + k_geo_pick */,
    VC_K_TEMPORAL_VOTE /* k_temporal_vote */, VC_K_TEMPORAL_RANK /* k_count_groups, k_cc_wcount, k_cc_woff, k_temporal_new<votes only> */,
    VC_K_TEMPORAL_MERGE /* k_merge_old + k_temporal_new */,
    VC_K_GROW_MARK /* k_grow_mark: the new set's bits and counts */, VC_K_GROW_RANK /* k_grow_apply, k_count_groups, k_cc_wcount, k_cc_woff */,
    VC_K_GROW_MERGE /* k_merge_old + k_grow_new */
} vc_kernel_kind;
#define VC_KERNEL_KINDS 28
enum {
    VC_WORK_WORD_BOXES = 0,   /* 8-byte word boxes k_brick_words read (listed bricks x 64 words x cameras asked)           */
    VC_WORK_TABLE_ENTRIES,    /* 4-byte table entries the per-voxel level read (VC_MODE_LUT)                                */
    VC_WORK_PROJECTIONS,      /* float64 projections the per-voxel level did (VC_MODE_FUSED)                                */
    VC_WORK_EMIT_PROJECTIONS, /* float64 projections the record expansion did (VC_MODE_FUSED without the colour table)      */
    VC_WORK_BRICK_BOXES,      /* 8-byte brick boxes k_cull_bricks read                                                      */
    VC_WORK_FOOT_PROJECTIONS, /* float64 projections k_carve_foot did (vc_carve_footprint)                                  */
    VC_WORK_FOOT_UNION_SKIPS, /* (word, camera) visits of k_carve_foot that the union-box count ended: no foreground under  */
                              /* the whole word, the camera fails its 64 voxels at once                                     */
    VC_WORK_FOOT_WORDS,       /* occupancy words k_carve_foot took                                                          */
    VC_WORK_DIST_CELLS,       /* cells of the boxes the distance transforms ran over (vc_hull_distance, vc_hull_morphology,    */
                              /* vc_hull_grow, vc_hull_compare with VC_COMPARE_DISTANCE),                                     */
                              /* one count per transform: each of its three passes reads and writes that many 8-byte values   */
    VC_WORK_DIST_LINES        /* lines k_dist_y and k_dist_env walked                                                        */
};
#define VC_WORK_KINDS 10

typedef struct {
    float carve_ms;     /* the carve kernels alone (HIP events on the context's stream).  carve_ms, first_ms, compact_ms
                           and prep_ms are measured for vc_carve calls and, with option timing_detail = 1, for
                           vc_carve_begin steps: an event between two kernels costs the stream ~10 us, so pipelined
                           steps record only the events they need anyway (emit_ms comes from those) */
    float compact_ms;   /* scan + emit kernels                                         */
    float gather_ms;    /* RCCL all-gather (vc_allgather)                              */
    float lut_ms;       /* last vc_build_lut                                           */
    float h2d_ms;       /* last vc_upload_masks / vc_upload_frame incl. bit-packing    */
    uint64_t voxels;    /* voxels of this rank's slab                                  */
    uint64_t survivors; /* survivors of the last carve (this rank)                     */
    uint32_t carve_launches; /* carve kernel launches since vc_timing_reset            */
    float carve_ms_sum; /* summed carve kernel time since vc_timing_reset              */
    float first_ms;     /* VC_MODE_LUT: the first-camera streaming kernel of the last carve */
    float first_ms_sum; /* summed since vc_timing_reset                                 */
    float exchange_ms;  /* vc_allgather, compact form: pack + RCCL part of gather_ms         */
    float gather_ms_sum; /* summed since vc_timing_reset                                */
    uint32_t gathers;   /* vc_allgather calls since vc_timing_reset                      */
    float prep_ms;      /* per-frame preparation queued in front of the last carve (bit-pack, boxes, grids, camera order);
                           measured only with option timing_detail = 1 (one more event on the carve stream) */
    float prep_ms_sum;  /* summed since vc_timing_reset                                  */
    uint32_t preps;     /* carve steps that had to prepare their frame set since vc_timing_reset */
    uint32_t preps_timed; /* ... of which prep_ms_sum holds the time                     */
    float emit_ms;      /* record expansion of the last step: the launch's own begin .. end (the events ride on the launch) */
    float emit_ms_sum;  /* summed since vc_timing_reset                                  */
    uint32_t emit_launches;
    /* Option timing_detail = 1: every kernel of a step carries its own begin / end events (on its launch: no extra packet on
     * the stream) and the kernels count the work they do.  Index = vc_kernel_kind; summed since vc_timing_reset. */
    float kernel_ms_sum[VC_KERNEL_KINDS];
    uint32_t kernel_launches[VC_KERNEL_KINDS];
    /* work[VC_WORK_*]: what the kernels of those steps actually touched (counted on the device, lanes that really asked);
     * valid when no step is in flight */
    uint64_t work[VC_WORK_KINDS];
    float visible_ms;   /* last vc_color_visible: its kernels, fill of the maps to the last colour (HIP events on the context's stream) */
    float thin_ms;      /* last vc_hull_thin: HIP events around the whole call */
    float thin_kernel_ms; /* ... and, with option timing_detail = 1, the sum of its mark, sub-step, list and row kernels' own
                           begin .. end (0 otherwise): thin_ms minus this is the time the stream spent between them */
    uint32_t thin_launches; /* the kernels of that sum */
} vc_timing_t;

/* ---- lifetime ------------------------------------------------------------------ */
int vc_device_count(int *n_out);
int vc_create(int device, vc_ctx **out);
int vc_destroy(vc_ctx *ctx);
const char *vc_last_error(const vc_ctx *ctx);      /* ctx may be NULL: last create error */
int vc_synchronize(vc_ctx *ctx);

/* ---- geometry: replaces create_voxel_volume, voxel_reconstruction.py:35-59 ------ */
/* bounds = {x_min,x_max,y_min,y_max,z_min,z_max}.  No point array is materialised:
 * kernels regenerate the np.linspace coordinates from the index. */
int vc_set_grid(vc_ctx *ctx, uint32_t nx, uint32_t ny, uint32_t nz, const double bounds[6]);
/* This rank's block of the grid: iz in [z0, z1) (multi-GPU z-slab split).  Default all. */
int vc_set_slab(vc_ctx *ctx, uint32_t z0, uint32_t z1);
/* The three np.linspace axes as the device uses them (tests; out arrays of nx, ny, nz). */
int vc_get_axes(vc_ctx *ctx, double *xs, double *ys, double *zs);

/* ---- cameras: replaces load_config_info, voxel_reconstruction.py:10-32 ---------- */
/* K9: [C,9] row-major camera matrices; dist5: [C,5] (k1,k2,p1,p2,k3); R9: [C,9] rotation
 * matrices (host does Rodrigues so fixtures pin R); t3: [C,3]; H, W: mask size. */
int vc_set_cameras(vc_ctx *ctx, uint32_t n_cameras, const double *K9, const double *dist5,
                   const double *R9, const double *t3, uint32_t H, uint32_t W);

/* ---- per-frame inputs: the fg_masks / images arguments of ------------------------
 *      update_visible_voxels_and_extract_colors, voxel_reconstruction.py:89 --------- */
/* masks: u8 [C,H,W], foreground where > 0 (line 112).  slot selects one of the resident frame sets (0..63, created
 * on first use).  ASYNCHRONOUS: the bytes are copied to a page-locked staging buffer and from there to the device
 * on an upload stream of their own, so the call returns at once and the copy runs beside the carve in flight; the
 * caller's buffer is free when the call returns.  Everything derived from the bytes (bit masks, foreground boxes,
 * cropped block grids, camera visiting order, images in the records' byte order) is made ON THE DEVICE by two kernels queued in front of
 * the first vc_carve / vc_carve_begin that uses the slot -- no host round trip anywhere. */
int vc_upload_masks(vc_ctx *ctx, uint32_t slot, const uint8_t *masks);
/* The byte masks and images resident in `slot` are to be taken as NEW input: the next carve on the slot derives
 * everything from them again (what a producer that writes the masks on the device, or a benchmark that wants every
 * step to pay for its own preparation, calls instead of uploading the same bytes again). */
int vc_touch_masks(vc_ctx *ctx, uint32_t slot);
/* Tail of extract_foreground_mask on the device (background_subtraction.py:195-206): per camera,
 * optional 2x2 MORPH_OPEN then 2x2 MORPH_CLOSE applied to the byte masks of every following
 * vc_upload_masks, before the final > 0 binarisation.  Arrays of C flags, NULL = none. */
int vc_set_mask_postfilter(vc_ctx *ctx, const uint8_t *open2x2, const uint8_t *close2x2);
/* The device's binarised mask of one camera as u8 [H,W] in {0,255} (tests). */
int vc_fetch_mask(vc_ctx *ctx, uint32_t slot, uint32_t cam, uint8_t *out);
/* bgr: u8 [H,W,3] image of camera cam (0-based) for colour sampling (lines 119-122).  Asynchronous like
 * vc_upload_masks. */
int vc_upload_frame(vc_ctx *ctx, uint32_t slot, uint32_t cam, const uint8_t *bgr);

/* ---- lookup table: replaces create_lookup_table, voxel_reconstruction.py:62-86 --- */
/* Projects this rank's slab once into int32 [C][n]: int(y)*W + int(x), or -1 when the
 * float coordinates fail the bounds test of line 110.  Needed by VC_MODE_LUT only. */
int vc_build_lut(vc_ctx *ctx);
int vc_fetch_lut(vc_ctx *ctx, uint32_t cam, int32_t *out);   /* n entries, voxel order */
/* The way back: replaces the pickled lookup table the reference can load instead of rebuilding it (load_lookup_table,
 * assignment.py:12-15).  One camera's n entries in voxel order, exactly what vc_fetch_lut gives out; once all cameras of
 * the context have been handed in the table is adopted (tile order, word and brick boxes reduced from it) and VC_MODE_LUT
 * runs on it.  Entries outside [-1, H*W) count as -1.  The host side (CarveEngine.save_lut / load_lut) wraps the table
 * with grid, slab, bounds, mask size and a digest of the camera parameters and refuses a file that does not match. */
int vc_upload_lut(vc_ctx *ctx, uint32_t cam, const int32_t *lut);
/* Device projection of arbitrary points with camera cam: uv = [n,2] float64 (tests). */
int vc_project(vc_ctx *ctx, uint32_t cam, const double *xyz, uint64_t n, double *uv);

/* ---- the hot path: replaces update_visible_voxels_and_extract_colors (:89-124) ----
 *      plus the selection loop of set_voxel_positions, assignment.py:116-133 -------- */
/* Keeps voxels seen by >= min_views cameras (reference: 4 of 4).  color_cam is the
 * 0-based camera whose image colours the survivors (reference key 2 -> index 1), or
 * -1 for none.  Leaves the ordered survivor records on the device; *n_out = count. */
int vc_carve(vc_ctx *ctx, uint32_t slot, uint32_t min_views, int color_cam, int mode,
             uint32_t flags, uint64_t *n_out);
/* The same step split in two so that step i+1 is queued on the device before the host collects
 * step i (no idle gap between steps).  At most THREE steps may be in flight (with two, the host cannot queue step i + 1
 * before it has collected step i - 1, whose record expansion ends about when the carve of step i does: the carve stream would
 * idle for the host's round trip); vc_carve_end completes the OLDEST one, whose records are then what vc_fetch_* /
 * vc_allgather read.  The steps rotate through three sets of result buffers: a vc_carve_begin that is queued into the set
 * holding the collected result (the third one after it was issued) takes it away -- fetch before that call; afterwards the
 * vc_fetch_* functions fail with VC_ERR_ARG until the next vc_carve_end.
 * min_views > n_cameras is legal and yields the empty result (as the reference's threshold test would).
 * Steps in flight may name different colour cameras.  With option fused_color_table = 1 (the default) a VC_MODE_FUSED step colours
 * its survivors from ONE table over the whole grid, projected for one camera at a time: a vc_carve_begin with another color_cam
 * projects its camera's table into the same buffer, on the device behind the last record expansion that was handed the old one
 * (a stream wait on that step's {done} event; the host does not wait, and a step with the camera of the step before it queues
 * nothing more than it did).  A step whose record buffer overflowed and whose table has been replaced since projects its survivors
 * itself when vc_carve_end expands it again, as with fused_color_table = 0: the same bytes.  VC_MODE_LUT reads a table per
 * camera. */
int vc_carve_begin(vc_ctx *ctx, uint32_t slot, uint32_t min_views, int color_cam, int mode, uint32_t flags);
int vc_carve_end(vc_ctx *ctx, uint64_t *n_out);
/* Footprint carve: a camera passes a voxel by the foreground count of the pixel box its whole CELL projects to, not by the one
 * pixel under its centre (vc_carve, which stays the default rule and is untouched by this call).  No counterpart in the
 * reference; restated in tests/footprint_np.py.  Projection is the carve's float64 projection (csrc/vc_device.h), no
 * behind-camera cull.
 *  1. Cell.  Per axis with n cells, bounds lo, hi and centres c[k] (vc_get_axes): h = 0.5 * ((hi - lo) / (n - 1)) (0 when
 *     n == 1); lattice L[k] = c[k] - h for k < n, L[n] = c[n-1] + h.  Voxel (ix, iy, iz) has the 8 corners L[i], L[i+1] per
 *     axis: neighbours share corners bit for bit.
 *  2. Box.  The 8 corners and the centre are projected; u_lo, u_hi, v_lo, v_hi are the per-coordinate min / max over the 9
 *     points with NaNs ignored (fmin / fmax).  A camera for which the centre's u or v is NaN does not see the voxel.
 *     bx0 = clamp(floor(u_lo), -1, W), bx1 = clamp(floor(u_hi), -1, W), by0, by1 likewise with H (clamped in float64, then
 *     converted).  area = (bx1 - bx0 + 1) * (by1 - by0 + 1); cnt = foreground pixels of the slot's prepared mask (what
 *     vc_fetch_mask returns) inside the box intersected with the image.
 *  3. Test.  VC_FOOT_ANY: cnt > 0.  VC_FOOT_COVER: cnt * 256 >= q * area in 64-bit integers, q in 1..256; q = 256 ("all") asks
 *     for a box inside the image that is all foreground.  For every camera set any >= centre >= all as sets of voxels.
 *  4. T = cameras that pass; a voxel is kept when T >= min_views and T >= 1.  Records in ascending linear index, 8 bytes as
 *     vc_carve's.  Colour and seen: the colour camera's pixel under the voxel's CENTRE whenever the centre is inside its image
 *     (the mask is not consulted), seen = 1; else 0, 0, 0 and seen = 0.  Occupancy words and, with VC_FLAG_VIEWMASK, the per-
 *     voxel camera bits (bit c = camera c passes) as vc_carve leaves them; vc_set_slab is honoured.
 * The count of a box is four loads from a summed-area table per camera ((H+1) x (W+1) u32, built on the device from the slot's
 * prepared bits the first time a footprint carve uses that preparation of the slot, kept until the slot is prepared again;
 * callers of vc_carve alone never allocate one).  Synchronous; the result is what every vc_fetch_* and post-carve pass reads,
 * exactly as after vc_carve (vc_surface_mesh keeps testing the CENTRE rule: vertices it cannot bracket stay at the midpoint).
 * flags: VC_FLAG_VIEWMASK | VC_FLAG_NO_RECORDS.  VC_ERR_ARG (with a message, nothing launched) for a rule other than
 * VC_FOOT_ANY / VC_FOOT_COVER, q outside 1..256, steps in flight, no grid / cameras / masks in the slot, a colour camera out of
 * range. */
int vc_carve_footprint(vc_ctx *ctx, uint32_t slot, uint32_t min_views, int color_cam, uint32_t rule, uint32_t q, uint32_t flags,
                       uint64_t *n_out);
/* Survivors of the last carve: idx u32 [S] (global linear index, ascending), rgb u8 [S,3]
 * (RGB order, i.e. the reference's BGR[::-1]) and seen u8 [S] (1 if the colour camera
 * sees the voxel -- the reference raises KeyError when it does not).  Any may be NULL. */
int vc_fetch(vc_ctx *ctx, uint32_t *idx, uint8_t *rgb, uint8_t *seen);
/* Raw 8-byte records {u32 idx, u8 r, g, b, seen} of the last carve (S of them). */
int vc_fetch_records(vc_ctx *ctx, uint64_t *records);
/* Page-locked host buffers for the fetch destinations (PCIe-rate read-back). */
int vc_host_alloc(vc_ctx *ctx, uint64_t bytes, void **out);
int vc_host_free(vc_ctx *ctx, void *ptr);
/* Per-voxel camera bitmask u16 [n] of the last carve run with VC_FLAG_VIEWMASK. */
int vc_fetch_viewmask(vc_ctx *ctx, uint16_t *viewmask);
/* Dense occupancy of the last carve: ceil(n/64)*8 bytes, bit (j & 7) of byte j >> 3 for
 * slab-local voxel j (consumer shape of assignment.py:143-146). */
int vc_fetch_occupancy(vc_ctx *ctx, uint8_t *bits);

/* ---- occlusion-aware colouring (no reference counterpart: the reference colours every survivor from camera key 2,
 *      assignment.py:133) ----------------------------------------------------------------------------------------------
 * vc_color_visible recolours the records of the current carve result IN PLACE from every camera that sees each surface voxel,
 * using the images of frame set `slot` (every camera needs one: vc_upload_frame or vc_foreground_to_slot), and keeps per survivor
 * the mask of those cameras.  Opt-in: nothing else changes, and the next carve produces the colour camera's colours again.
 * The contract, bit for bit (tests/visible_np.py restates it; projection = the carve's float64 projection, same operation order,
 * no contraction; xs, ys, zs = the grid's linspace axes):
 *   1 surface: a survivor with at least one of its 6 face neighbours (iy +- 1 = index i +- 1, ix +- 1 = i +- ny, iz +- 1 =
 *     i +- nx ny) not a survivor or outside the grid.  Other survivors are never visible.
 *   2 voxel box: half extents hx = ((x_max - x_min) / (nx - 1)) / 2 (0 when nx = 1), likewise hy, hz; the 8 corners are
 *     xs[ix] +- hx, ys[iy] +- hy, zs[iz] +- hz, one float64 add or subtract each.
 *   3 depth maps: one u32 [H W] per camera, filled with the bits of +inf.  For surface voxel v and camera c: d = camera z of the
 *     centre, R20 X + R21 Y + R22 Z + t2 left to right in float64.  Unless d > 0 and every corner's camera z > 0, v does not
 *     splat into c; nor does it when any of umin, umax, vmin, vmax over the 8 projected corners is not finite.  Otherwise the
 *     pixels x0 = max(floor(umin), 0) .. x1 = min(floor(umax), W - 1), y0 = max(floor(vmin), 0) .. y1 = min(floor(vmax), H - 1)
 *     (if any) each take atomicMin with bits((float)d) -- positive floats order like their bits: the maps are deterministic.
 *   4 visibility: surface voxel v is visible in camera c when d > 0, its centre (u, v) passes the carve's in-image test
 *     (0 <= v < H and 0 <= u < W on the floats) and (float)d <= zmap_c[int(v) W + int(u)] + tol (the add in float32).
 *   5 colour: a survivor visible in a non-empty set V of cameras gets, per channel, (sum over V of ch_c + |V| / 2) / |V| in
 *     integers, ch_c = camera c's pixel int(v) W + int(u); with V empty the record keeps its RGB.  The seen byte never changes.
 * depth_tolerance (tol) >= 0; CarveEngine.color_visible's default is the voxel diagonal (float)sqrt((2hx)^2 + (2hy)^2 + (2hz)^2).
 * flags must be 0.  VC_ERR_ARG (with a message) when: there is no carve result, steps are in flight, the carve ran with
 * VC_FLAG_NO_RECORDS, a camera of the slot has no image, tol is negative or NaN, the slab is narrower than the grid or a
 * communicator of more than one rank is attached (multi-GPU visibility is out of scope).  S = 0 is no error.  Synchronous: the
 * records are recoloured when the call returns.
 * vc_fetch_visibility: u16 [S] in record order, bit c = visible in camera c (0 for survivors that are not surface voxels).
 * vc_fetch_depth: camera cam's map as float [H W] (+inf where nothing splatted).  Both fail until vc_color_visible has run on
 * the current carve result; the next carve invalidates them. */
int vc_color_visible(vc_ctx *ctx, uint32_t slot, float depth_tolerance, uint32_t flags);
int vc_fetch_visibility(vc_ctx *ctx, uint16_t *vis);
int vc_fetch_depth(vc_ctx *ctx, uint32_t cam, float *out);

/* ---- photo-consistency carving (no reference counterpart: the reference keeps the visual hull) ------------------------------
 * vc_photo_carve refines the current carve result A1 (S0 records in ascending index order) by space carving in the style of
 * voxel colouring / GVC: a surface voxel that the cameras seeing it see in clearly different colours is removed, which exposes
 * the voxels behind it, and the test repeats.  Opt-in; the next carve restores the visual hull.  The contract, bit for bit
 * (tests/photo_np.py restates it).  Inputs: frame set `slot` (every camera needs an image), tol (depth_tolerance, meaning and
 * default as vc_color_visible's), T = var_threshold (u32, squared 8-bit levels), m = min_views (2 <= m <= C), R = max_rounds
 * (1 <= R <= 255).  For round r = 1 .. R:
 *   1 the surface, the depth maps and the visible set V of every surface voxel of A_r: items 1-4 of vc_color_visible applied to A_r;
 *   2 for a surface voxel with n = |V|, ch_c = camera c's RGB at pixel int(v) W + int(u) (item 5's sample), per channel k
 *     s_k = sum over V of ch, q_k = sum over V of ch^2, and D = sum_k (n q_k - s_k^2) in exact integers (= n^2 x the sum of the
 *     per-channel population variances);
 *   3 the voxel is inconsistent iff n >= m and D > T n^2 (64-bit integers, no floating point); I_r = the inconsistent voxels;
 *   4 I_r empty: converged at round r, stop.  Otherwise A_{r+1} = A_r \ I_r and every voxel of I_r gets round number r.  All
 *     removals of a round are decided from A_r alone (Jacobi); the order voxels are visited in never matters.
 * F = A_r when the loop converged at round r, else A_{R+1}.  After the call:
 *   records: F's records in ascending index order, coloured exactly as vc_color_visible colours the input records restricted to F
 *     (interior voxels keep their RGB, the seen byte never changes); vc_fetch_visibility / vc_fetch_depth return what
 *     vc_color_visible on F gives; vc_fetch_occupancy returns F; vc_fetch, vc_fetch_records and the survivor count give |F|;
 *     vc_pack_entries / vc_allgather (one rank) pack F.  vc_fetch_viewmask and vc_expand_entries stay the silhouette carve's
 *     (the view mask of every voxel; colours from the colour camera).
 *   vc_fetch_photo_rounds: u8 [S0], the round number of each input record in input order, 0 = kept.  It fails until a photo carve
 *     has run on the current result; the next carve invalidates it.  vc_photo_carve may run again on F, with F as its input.
 * stats: rounds = rounds evaluated (the empty round that shows convergence counts), converged = 1 if the loop stopped on an
 * empty round, survivors_before = S0, survivors_after = |F|, photo_ms = HIP events around the whole call.  One 4-byte read-back
 * per round (the round's removal count).  VC_ERR_ARG (with a message) in every case vc_color_visible refuses, and when m < 2,
 * m > C, R = 0, R > 255, flags != 0 or stats == NULL.  S0 = 0 is no error (converged at round 1).  Synchronous. */
typedef struct {
    uint32_t rounds;
    uint32_t converged;
    uint64_t survivors_before, survivors_after;
    float photo_ms;
} vc_photo_stats_t;
int vc_photo_carve(vc_ctx *ctx, uint32_t slot, float depth_tolerance, uint32_t var_threshold,
                   uint32_t min_views, uint32_t max_rounds, uint32_t flags, vc_photo_stats_t *stats);
int vc_fetch_photo_rounds(vc_ctx *ctx, uint8_t *rounds);   /* u8 [survivors_before] */

/* ---- connected components of the hull (no reference counterpart: the reference keeps every survivor) ---------------------------
 * vc_hull_components labels the connected components of the current carve result A (S0 records in ascending linear index i) and
 * removes the survivors of the components that fail a size rule: specks of mask noise that every camera happens to agree on
 * survive the carve as small clumps beside the figure.  Opt-in; the next carve restores the visual hull.  The contract, bit for
 * bit (tests/components_np.py restates it).  Inputs: connectivity N in {6, 18, 26} (the neighbourhood of
 * scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3): face, + edge, + corner neighbours), min_voxels (0 and 1: no floor),
 * keep_largest (0: no limit), flags = 0.
 *   1 two survivors are connected when they are N-neighbours in (ix, iy, iz), no wrap-around (i and i + 1 are not neighbours
 *     when (i + 1) % ny == 0);
 *   2 a component's label is its smallest linear index (the index of its first record), its size the number of its voxels,
 *     its box the inclusive lo[3], hi[3] of its (ix, iy, iz);
 *   3 rank orders the components by size descending, then label ascending; a component is kept iff size >= min_voxels and,
 *     when keep_largest > 0, rank < keep_largest.
 * After the call:
 *   records, count, occupancy: the kept survivors only, records in ascending order with colour and seen byte unchanged;
 *     vc_fetch_occupancy, vc_fetch, vc_fetch_records, vc_pack_entries / vc_allgather (one rank), vc_marching_cubes(volume NULL)
 *     see the filtered hull.  vc_fetch_viewmask and vc_expand_entries stay the silhouette carve's.  Visibility, depth maps and
 *     photo rounds of an earlier vc_color_visible / vc_photo_carve fail until those run again.
 *   vc_fetch_component_labels: u32 [S0], the label of each input record in input order.
 *   vc_fetch_components: vc_component_t [components] in ascending label.
 *   Both fail until the pass has run on the current result; vc_hull_components may run again on its own output.
 * stats: components, components_kept, survivors_before = S0, survivors_after, largest (size of the largest component, 0 on an
 * empty hull), components_ms = HIP events around the whole call.  One read-back in the middle (the number of components).
 * VC_ERR_ARG (with a message) when there is no carve result, steps are in flight, the carve ran with VC_FLAG_NO_RECORDS, a
 * communicator of more than one rank is attached, the slab is narrower than the grid, N is not 6, 18 or 26, flags != 0 or
 * stats == NULL.  S0 = 0 is no error (no components).  Synchronous. */
typedef struct {
    uint32_t components, components_kept;
    uint64_t survivors_before, survivors_after;
    uint32_t largest;          /* size of the largest component, 0 on an empty hull */
    float    components_ms;    /* HIP events around the whole call */
} vc_component_stats_t;
typedef struct { uint32_t label, size, lo[3], hi[3], kept, reserved; } vc_component_t;

int vc_hull_components(vc_ctx *ctx, uint32_t connectivity, uint64_t min_voxels, uint32_t keep_largest,
                       uint32_t flags, vc_component_stats_t *stats);
int vc_fetch_component_labels(vc_ctx *ctx, uint32_t *labels);      /* u32 [survivors_before], input record order */
int vc_fetch_components(vc_ctx *ctx, vc_component_t *out);         /* [components], ascending label */

/* ---- Euclidean distance field of the hull; erosion and opening by a ball in world units (no reference counterpart) ------------
 * vc_hull_distance computes the exact squared Euclidean distance transform of the current carve result as vc_fetch_occupancy sees
 * it (vc_photo_carve, vc_hull_components and the footprint rules included); vc_hull_morphology erodes or opens the hull by a ball
 * given in world units, which an index-space structuring element cannot do on an anisotropic grid.  The contract, bit for bit
 * (tests/distance_np.py restates it).  Everything is unsigned 64-bit integer arithmetic and a minimum over a set, so the result
 * does not depend on evaluation order.
 *   1 input: a voxel is (ix, iy, iz) with i = (iz nx + ix) ny + iy; ON = survivor, OFF = any other voxel of the grid.
 *   2 metric: per axis a, s_a = (max_a - min_a) / (n_a - 1) in float64 and q_a = llrint(s_a * 1000.0) micrometres.
 *     VC_ERR_ARG when an axis is shorter than 2, some q_a lies outside 1 .. 2^20 or (n_a + 1) q_a > 2^30 for some axis; with
 *     those bounds every d2 below is < 2^62.  VC_ERR_ARG also when an axis is longer than 4096 cells (a limit of this build: the
 *     kernels hold a line's positions in 16 bits and a y line's site words in shared memory).  d2(v, w) = (q_x dix)^2 + (q_y diy)^2 + (q_z diz)^2 in um^2.
 *   3 inside field: D_in(v) = min over sites w of d2(v, w).  The sites are the OFF voxels and, with VC_DIST_BORDER_OFF, one virtual
 *     OFF layer around the grid: every position with exactly one coordinate equal to -1 or n_a and the other two inside the grid.
 *     D_in of an OFF voxel is 0; with no site at all (a full grid, border open) D_in is UINT64_MAX.
 *   4 outside field (only with VC_DIST_OUTSIDE): D_out(v) = min over ON voxels w of d2(v, w); 0 on ON voxels, UINT64_MAX when the
 *     hull is empty; the border never contributes.
 *   5 erosion by r2 (um^2): E = { v ON : D_in(v) > r2 }.
 *   6 opening by r2: O = { v ON : min over e in E of d2(v, e) <= r2 }; empty when E is; r2 = 0 is the identity whenever a site
 *     exists.
 *   7 after vc_hull_morphology: records, count and occupancy hold the kept survivors only (E for VC_MORPH_ERODE, O for
 *     VC_MORPH_OPEN), records in ascending order with colour and seen byte unchanged -- the hand-over vc_hull_components makes.
 *     vc_fetch_viewmask and vc_expand_entries stay the silhouette carve's.  Visibility, depth maps, photo rounds, component labels
 *     and a stored distance field fail until their pass runs again.  The next carve restores the visual hull.
 * vc_fetch_record_distance: u64 [S], D_in of each record in record order.  vc_fetch_distance: the dense field, u64 [N] in linear
 * index, which = 0 inside, 1 outside (needs VC_DIST_OUTSIDE).  The fetch calls fail until vc_hull_distance has run on the current
 * result, and again after anything that changes the result.  vc_hull_morphology computes what it needs itself.
 * stats (required): survivors; sites_inside_box (a diagnostic: site cells of the box the inside transform ran over, the hull's
 * index box grown by one cell per side); max_d2 = max D_in over ON, 0 on an empty hull; q = q_x, q_y, q_z; eroded = |E|;
 * distance_ms / morph_ms = HIP events around the whole call.  flags of vc_hull_morphology: VC_DIST_BORDER_OFF only.
 * VC_ERR_ARG (with a message) when there is no carve result, steps are in flight, the carve ran with VC_FLAG_NO_RECORDS, the slab
 * is narrower than the grid, a communicator of more than one rank is attached, flags or op are unknown, stats == NULL or the
 * metric is out of range (2).  An allocation failure returns VC_ERR_OOM and leaves the result untouched.  S = 0 is no error.
 * Synchronous, one read-back in the middle (the survivors' box). */
#define VC_DIST_BORDER_OFF 1u
#define VC_DIST_OUTSIDE    2u
#define VC_MORPH_ERODE 0u
#define VC_MORPH_OPEN  1u
typedef struct {
    uint64_t survivors, sites_inside_box /* diagnostic */, max_d2 /* max D_in over ON, 0 if none */;
    uint64_t q[3];                  /* x, y, z in um */
    float distance_ms;              /* HIP events around the whole call */
} vc_distance_stats_t;
typedef struct {
    uint64_t survivors_before, eroded /* |E| */, survivors_after, max_d2;
    uint64_t q[3];
    float morph_ms;
} vc_morph_stats_t;
int vc_hull_distance(vc_ctx *ctx, uint32_t flags, vc_distance_stats_t *stats);
int vc_fetch_record_distance(vc_ctx *ctx, uint64_t *d2);           /* [S], D_in of each record, record order */
int vc_fetch_distance(vc_ctx *ctx, uint32_t which, uint64_t *d2);  /* dense [N] in linear index; 0 = inside, 1 = outside */
int vc_hull_morphology(vc_ctx *ctx, uint32_t op, uint64_t r2, uint32_t flags, vc_morph_stats_t *stats);

/* ---- dilation and closing of the hull by a ball in world units: the growing half of the morphology (no reference counterpart) --
 * Every other pass over a carve result can only take voxels away.  vc_hull_grow ADDS survivors: it dilates or closes the current
 * carve result, as vc_fetch_occupancy sees it, by a ball of squared radius r2 in um^2, and creates the records of the voxels it
 * adds.  A closing fills what is narrower than the ball -- the tunnel that a hole in one camera's mask carves through the figure --
 * and leaves the rest of the hull as it is.  The contract, bit for bit (tests/closing_np.py restates it).  Unsigned 64-bit integers
 * only; the metric q_a and d2 are exactly those of vc_hull_distance (items 1 and 2 above), with the same refusals.
 *   1 dilation: Dl = { v in the grid : min over ON voxels w of d2(v, w) <= r2 }.  Empty for an empty hull.  Clipped to the grid:
 *     there are no voxels outside it.
 *   2 closing: C = { v in Dl : min over grid voxels u not in Dl of d2(v, u) > r2 }; when every grid voxel is in Dl the condition
 *     holds and C is the whole grid.  The border is open: nothing outside the grid is a site.  With these two definitions dilation
 *     and erosion are an adjunction on the subsets of the grid, so hull <= C <= Dl, the closing is idempotent (closing C again
 *     adds nothing) and increasing (A <= B gives C(A) <= C(B)), and r2 = 0 is the identity for both ops.
 *   3 records after the call: records, count and occupancy describe Dl (VC_GROW_DILATE) or C (VC_GROW_CLOSE), in ascending linear
 *     index.  A record that existed keeps its 8 bytes.  An added voxel's record takes item 4 of vc_carve_footprint: the colour
 *     camera's pixel under the voxel's CENTRE whenever the centre is inside its image, by the carve's float64 projection and
 *     in-image test (the mask is not consulted), seen = 1; otherwise 0, 0, 0 and seen = 0, which is also what a carve without a
 *     colour camera gives.  The colour comes from the images of the carve's frame set as that carve saw them: when the slot has
 *     been prepared again since (new masks or images and a later preparation), the call is refused, as vc_surface_mesh is.
 *   4 other readers: vc_fetch_viewmask and vc_expand_entries stay the silhouette carve's.  Visibility, depth maps, photo rounds,
 *     component labels and a stored distance field fail until their pass runs again; a call that adds nothing (r2 = 0, a second
 *     closing, an empty hull) leaves the result and with it the first four valid, and drops only the stored distance field,
 *     whose buffer the transforms use (on an empty hull no transform runs, and the stored field stays valid too).  The next
 *     carve restores the visual hull.
 *     Everything that reads the step sees the grown hull exactly as it sees an opened one.  vc_surface_mesh keeps its own
 *     contract: edges at added voxels are not bracketed by the centre test and stay at the midpoint, as for VC_FOOT_ANY.
 *   5 VC_ERR_ARG (with a message, nothing launched) when there is no carve result, steps are in flight, the carve ran with
 *     VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached, op is unknown,
 *     flags != 0, stats == NULL, the metric is out of range or the slot has been prepared again.  An allocation failure returns
 *     VC_ERR_OOM and leaves the result untouched: the added voxels are counted, and every buffer sized, before anything changes.
 *     (The result: records, count, occupancy.  A stored distance field and an earlier call's added bytes are gone after a
 *     failed call too: vc_fetch_distance and vc_fetch_grown fail until their pass runs again.)
 *     S = 0 is no error and stays empty.
 * The transforms run over the survivors' index box grown per axis by g_a + 1 cells, g_a = isqrt(r2) / q_a, and clipped to the
 * grid (DESIGN.md section 8 item 13 has the argument); a large radius makes the box the grid.
 * stats (required): survivors_before; dilated = |Dl|; survivors_after; added = survivors_after - survivors_before; box_cells =
 * cells of that box; q; grow_ms = HIP events around the whole call.  vc_fetch_grown: u8 [survivors_after] in record order, 1 =
 * the record was created by the last vc_hull_grow; fails once a carve or a pass that removes survivors has run since.
 * Synchronous, two read-backs in the middle (the survivors' box, the count of added voxels). */
#define VC_GROW_DILATE 0u
#define VC_GROW_CLOSE  1u
typedef struct {
    uint64_t survivors_before, dilated /* |Dl| */, survivors_after, added, box_cells;
    uint64_t q[3];
    float grow_ms;
} vc_grow_stats_t;
int vc_hull_grow(vc_ctx *ctx, uint32_t op, uint64_t r2, uint32_t flags /* must be 0 */, vc_grow_stats_t *stats);
int vc_fetch_grown(vc_ctx *ctx, uint8_t *added);   /* u8 [S_after], record order: 1 = created by the last vc_hull_grow */

/* ---- a vote of each voxel over the last frames' hulls (no reference counterpart) ------------------------------------------------
 * Every other pass works on one frame.  Mask noise differs in every frame of a video, so voxels appear and vanish between carves
 * while the figure stands still; vc_hull_temporal keeps the last `window` hulls on the device and replaces the current result by
 * their vote.  It puts back what a momentary mask hole carved out and drops specks that live for one frame, with no radius and no
 * size threshold.  The contract, bit for bit (tests/temporal_np.py restates it).  Integers only.
 *   1 push: H_t is the current result's occupancy, as vc_fetch_occupancy sees it when the call starts.  It becomes the newest of a
 *     ring of `window` snapshots on the device.  m = min(pushes since the last reset, window).
 *   2 count: c(v) = the number of j in 0 .. m - 1 with v in H_{t-j}; c(v) <= 15.
 *   3 thresholds: 1 <= keep_off <= keep_on <= window <= VC_TEMPORAL_MAX_WINDOW.  on = ceil(keep_on m / window), off =
 *     ceil(keep_off m / window), in integers: they grow with the ring while it fills, and with m = 1 both are 1, so the first call
 *     after a reset returns the hull as it is.
 *   4 vote with hysteresis: P is the previous call's output, empty after a reset.  O_t = { v : c(v) >= on } + { v in P : c(v) >=
 *     off }.  keep_off = keep_on is the plain k-of-window vote; keep_on = window with keep_off = 1 gives a hull that is slow to
 *     take a voxel and slow to let it go.
 *   5 result after the call: records, count and occupancy describe O_t in ascending linear index.  A record of H_t & O_t keeps its
 *     8 bytes.  A voxel of O_t \ H_t gets a fresh record exactly as item 3 of vc_hull_grow colours one (the colour camera's pixel
 *     under the centre, by the carve's float64 projection and in-image test, seen = 1; else zeros).  Records of H_t \ O_t are
 *     dropped.  votes[r] = c of record r, added[r] = 1 for a fresh record.  Other readers follow item 4 of vc_hull_grow: when
 *     O_t = H_t nothing is invalidated and the result generation does not advance, otherwise every product of a pass is stale.
 *   6 stats: window; frames = m; on, off = the effective thresholds of this call; raw_changed = |H_t xor H_{t-1}| (0 when m = 1);
 *     out_changed = |O_t xor P|; added = |O_t \ H_t|; removed = |H_t \ O_t|; survivors_after = survivors_before + added -
 *     removed; temporal_ms = HIP events around the whole call.
 *   7 state: the ring and P survive carves, passes and results.  They are reset by vc_temporal_reset, by a change of grid, slab or
 *     cameras, and by a call whose `window` differs from the ring's.  keep_on and keep_off may change from call to call.
 *   8 one push per result: the call is refused when the current result is already the last call's output.  Carve again first.
 *     A pass that makes another result of it (erode, open, components, photo-consistency, a grow that adds voxels) lifts the
 *     refusal as a carve does, and that result is pushed as it stands.  So does vc_temporal_reset: the votes of the last call go
 *     with the ring (vc_fetch_temporal fails), and the current result may be pushed as the first hull of the new ring.
 *   9 VC_ERR_ARG (with a message, nothing launched, no state touched) when there is no carve result, steps are in flight, the
 *     carve ran with VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached,
 *     flags != 0, stats == NULL, window is 0 or above 15, keep_on or keep_off is out of range, the grid has more voxels than a u32
 *     index, the slot has been prepared again since the carve (as vc_hull_grow), or item 8 applies.
 *  10 an allocation failure returns VC_ERR_OOM and leaves result, ring and P as they were: the vote reads the result's words in
 *     place and writes O_t to a staging buffer; the counts are read back and every buffer is sized before anything is committed.
 *     Only then does the newest snapshot overwrite the ring's oldest slot (which the vote never reads), O_t go into the result's
 *     words, and the staging buffer become P.
 *  11 vc_fetch_temporal fails unless the current result is the last call's output; vc_fetch_temporal_history fails for age >= m.
 * Memory: (window + 2) nwords 8 bytes (0.94 GB at 1024^3 with window 5), allocated by the first call.  What it does not do: it lags
 * a moving figure by about window / 2 frames, there is no motion compensation (vc_hull_temporal_motion below has it; a ring that
 * call filled is started over by this one, as by another `window`), and multi-GPU is refused.
 * Synchronous, one read-back in the middle (the five counts). */
#define VC_TEMPORAL_MAX_WINDOW 15u
typedef struct {
    uint32_t window, frames /* m */, on, off /* the effective thresholds of this call */;
    uint64_t survivors_before, survivors_after, added, removed, raw_changed, out_changed;
    float temporal_ms;
} vc_temporal_stats_t;
int vc_hull_temporal(vc_ctx *ctx, uint32_t window, uint32_t keep_on, uint32_t keep_off, uint32_t flags /* must be 0 */, vc_temporal_stats_t *stats);
int vc_fetch_temporal(vc_ctx *ctx, uint8_t *votes, uint8_t *added);            /* u8 [S_after] each, record order; either may be NULL */
int vc_fetch_temporal_history(vc_ctx *ctx, uint32_t age, uint8_t *bits);       /* the raw hull pushed `age` calls ago, laid out as vc_fetch_occupancy */
int vc_temporal_reset(vc_ctx *ctx);

/* ---- set algebra on hulls: keep, load, combine and compare (no reference counterpart) --------------------------------------------
 * Every pass above works on the current carve result, which only a carve of the same context can make.  These calls give it a
 * second operand: VC_HULL_REGISTERS kept hulls on the device, a pass that combines the current result with one of them by a set
 * operation, and a pass that compares the two and changes nothing.  With them a saved reconstruction can be reloaded and measured,
 * thinned, meshed or rendered; a static scene subtracted; every frame clipped to a region; two sessions united; what moved between
 * two frames shown; and the difference of two hulls put in numbers.  Integers and bits only (tests/setops_np.py restates it).
 *
 * Kept hulls.  A register is empty or holds a hull of the current grid: its occupancy words (laid out as vc_fetch_occupancy, bits
 * at or beyond n zero), its voxel count and, optionally, its records (u64: index in the low 32 bits, R | G << 8 | B << 16 |
 * seen << 24 in the high 32, ascending index).  Registers survive carves, passes and results; a change of grid, slab or cameras
 * empties all of them, as it empties the ring of vc_hull_temporal.
 *   vc_hull_keep     the register becomes a copy of the current result, records included.  Refused as a pass is (no carve result,
 *                    steps in flight, VC_FLAG_NO_RECORDS, a narrower slab, a communicator of more than one rank).
 *   vc_hull_upload   exactly one of bits / records is non-NULL.  bits: laid out as vc_fetch_occupancy; the register then has no
 *                    records (n_records must be 0).  records: strictly ascending in the low 32 bits, every index below n; n_records
 *                    = 0 is the empty hull with records.  The device validates: a set bit at or beyond n, a record out of order, a
 *                    duplicate or an index at or beyond n returns VC_ERR_ARG.  The hull is built beside the register and swapped in
 *                    only when valid: a refused or failed upload leaves the register's previous content intact.  Needs a grid (the
 *                    whole grid as slab, no steps in flight, at most 2^32 voxels), not a carve result.
 *   vc_hull_release  empties the register and frees its memory; an empty register is no error.
 *   vc_fetch_kept    count and has_records (either may be NULL), the words into bits and the records into records (either may be
 *                    NULL: call with both NULL to size the buffers).  VC_ERR_ARG for an empty register, and for records of a
 *                    register that has none.
 *
 * vc_hull_combine.  A is the current occupancy as vc_fetch_occupancy sees it, B the register's.  VC_SETOP_COPY gives R = B,
 * VC_SETOP_AND A & B, VC_SETOP_OR A | B, VC_SETOP_ANDNOT A \ B, VC_SETOP_XOR the symmetric difference; R is restricted to the grid.
 *   1 result: records, count and occupancy describe R in ascending linear index.
 *   2 kept records: a record of A & R keeps its 8 bytes (but see 4).
 *   3 added voxels: a voxel of R \ A can only arise under COPY, OR or XOR.  When the register has records it takes B's 8 bytes
 *     verbatim; otherwise it gets a fresh record exactly as item 3 of vc_hull_grow colours one.  added[r] = 1 for these
 *     (vc_fetch_combined: u8 [survivors_after], record order).
 *   4 COPY from a register with records is a restore: every record of R is B's record verbatim, and added[r] = 1 only where the
 *     voxel was not in A.
 *   5 R = A: nothing is invalidated and the result generation does not advance, as a vote that equals its input.  Otherwise every
 *     product of a pass is stale, and a refusal of vc_hull_temporal under its item 8 is lifted.  A restore (4) always counts as
 *     another result, whether or not the sets differ: the records' bytes may.
 *   6 readers: vc_fetch_viewmask and vc_expand_entries stay the silhouette carve's.  Everything else reads R as an ordinary result.
 *   7 stats (required): survivors_before = |A|; other = |B|; common = |A & B|; survivors_after = |R|; added = |R \ A|; removed =
 *     |A \ R|; setop_ms = HIP events around the whole call.
 *   8 VC_ERR_ARG (with a message, nothing launched, no state touched) when there is no carve result, steps are in flight, the carve
 *     ran with VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached, op is
 *     unknown, flags != 0, stats == NULL, reg >= VC_HULL_REGISTERS, the register is empty, the grid has more voxels than a u32
 *     index, or -- only when fresh records would be coloured: the register has no records and op is COPY, OR or XOR -- the slot has
 *     been prepared again since the carve (as vc_hull_grow).
 *   9 an allocation failure returns VC_ERR_OOM and leaves result and registers as they were: R goes to a staging buffer, the
 *     counts are read back and every buffer is sized before anything is committed.
 * Synchronous, one read-back in the middle (the four counts).
 *
 * vc_hull_compare changes nothing: not the records, not the generation, not a stored vc_hull_distance field (it keeps a field
 * buffer of its own).  Always: a = |A|, b = |B|, common, only_a = |A \ B|, only_b = |B \ A|; the inclusive index box diff_lo,
 * diff_hi (x, y, z) of the symmetric difference, UINT32_MAX and 0 for an empty one; compare_ms.  With VC_COMPARE_DISTANCE, by
 * the metric of vc_hull_distance (its items 1 and 2, with the same refusals; q = the steps in um, else zeros): h2_ab = max over v
 * in A \ B of min over w in B of d2(v, w) in um^2, the directed Hausdorff distance squared (the voxels of A & B contribute 0); 0
 * when A \ B is empty, UINT64_MAX when A \ B is not and B is.  arg_ab = the smallest linear index that attains h2_ab, UINT32_MAX
 * when A \ B is empty.  h2_ba and arg_ba: the same with the roles swapped.  Without the flag the four are 0 and UINT32_MAX.
 * VC_ERR_ARG as items 8 of vc_hull_combine names them for a pass and a register, for unknown flags and stats == NULL.
 * Synchronous, one read-back in the middle (counts and boxes). */
#define VC_HULL_REGISTERS 4
#define VC_SETOP_COPY   0u
#define VC_SETOP_AND    1u
#define VC_SETOP_OR     2u
#define VC_SETOP_ANDNOT 3u
#define VC_SETOP_XOR    4u
#define VC_COMPARE_DISTANCE 1u
typedef struct {
    uint64_t survivors_before, other /* |B| */, common /* |A & B| */, survivors_after, added, removed;
    float setop_ms;
} vc_setop_stats_t;
typedef struct {
    uint64_t a, b, common, only_a, only_b;
    uint32_t diff_lo[3], diff_hi[3];    /* x, y, z, inclusive */
    uint64_t h2_ab, h2_ba;              /* um^2 */
    uint32_t arg_ab, arg_ba;            /* linear index */
    uint64_t q[3];
    float compare_ms;
} vc_compare_stats_t;
int vc_hull_keep(vc_ctx *ctx, uint32_t reg);
int vc_hull_upload(vc_ctx *ctx, uint32_t reg, const uint8_t *bits, const uint64_t *records, uint64_t n_records);
int vc_hull_release(vc_ctx *ctx, uint32_t reg);
int vc_fetch_kept(vc_ctx *ctx, uint32_t reg, uint8_t *bits /* NULL ok */, uint64_t *records /* NULL ok */, uint64_t *count, uint32_t *has_records);
int vc_hull_combine(vc_ctx *ctx, uint32_t op, uint32_t reg, uint32_t flags /* must be 0 */, vc_setop_stats_t *stats);
int vc_fetch_combined(vc_ctx *ctx, uint8_t *added);   /* u8 [S_after], record order: 1 = the voxel was not in A */
int vc_hull_compare(vc_ctx *ctx, uint32_t reg, uint32_t flags, vc_compare_stats_t *stats);

/* ---- block motion between consecutive hulls, and a hull warp (no reference counterpart) -------------------------------------------
 * The passes above work on one frame.  vc_hull_motion estimates where each part of the hull went between the hull of a register
 * (the previous frame, kept by vc_hull_keep) and the current result: one integer vector per block of b^3 voxels, by exhaustive
 * block matching on the two bit volumes.  Integers and bits only (tests/motion_np.py restates it).
 *
 * A is the current occupancy as vc_fetch_occupancy sees it, B the hull of register `reg`, bits only; both are empty outside the
 * grid.  Parameters: block edge b in {4, 8, 16}, apron a in 0..16, search range s in 1..8, with b + 2a + 2s <= 64 (one y row of a
 * block's search region is then at most one 64-bit word; 64 itself is allowed).
 *   1 blocks: the grid is cut into cubes of b^3 voxels, NB = ceil(n / b) per axis (grids need not be multiples of b); block index
 *     k = (bz NBx + bx) NBy + by, the voxels' own order.  A block is listed when its b^3 cells hold a voxel of A or of B.  Listed
 *     blocks come out in ascending k.
 *   2 cost: the window W(k) is the block grown by a cells per side, not clipped.  For d = (dx, dy, dz) in [-s, s]^3:
 *     cost(k, d) = |{ v in W(k) : A(v) != B(v - d) }|.  d is the displacement of the content from the old hull to the new one.
 *   3 the choice: the smallest cost wins; among equal costs the smallest dx^2 + dy^2 + dz^2; then the smallest (dz, dx, dy) in
 *     lexicographic order.  No order of evaluation shows.
 *   4 row per listed block (vc_motion_t): block; d (x, y, z); flags bit 0: some |component| of d equals s, so the motion may
 *     exceed the range; cost; cost0 = the cost at d = 0; count_a, count_b = the voxels of A and of B in the block proper; ties =
 *     how many displacements attain the smallest cost.  1 means the vector is determined; a window whose search region of B is
 *     solid or empty throughout gives d = 0 with ties = (2s + 1)^3: the aperture problem, reported and not hidden.
 *   5 stats (required): blocks, listed, moved (d != 0), unique (ties = 1), clipped (flag bit 0), cost0_sum and cost_sum (the
 *     change before and after compensation, over the listed blocks), a = |A|, b = |B|, motion_ms = HIP events around the call.
 *   6 vc_hull_motion changes nothing: not the records, not the result generation, not the register.
 *   7 VC_ERR_ARG (with a message, nothing launched) as item 8 of vc_hull_combine names them for a pass and a filled register, for
 *     flags != 0, stats == NULL, b, a or s outside their ranges, b + 2a + 2s > 64, and for more than 2^26 blocks.
 *   8 lifetime: the field is stale once the result generation advances (a carve or any pass that changes the survivors), once
 *     register `reg` is rewritten (vc_hull_keep, vc_hull_upload) or released, or once grid, slab or cameras change.
 *     vc_fetch_motion, vc_hull_warp and vc_paint_motion then return VC_ERR_ARG by name.  Colour passes (vc_color_visible,
 *     vc_paint_clusters, vc_paint_geodesic, vc_paint_motion) leave it valid.
 * vc_fetch_motion: the listed blocks into *count, their rows into rows (either may be NULL: call with rows NULL to size it).
 *
 * vc_hull_warp needs a current field made against register `src`, and dst != src.  It writes to register `dst` the prediction
 * P(v) = B(v - d_k) for v in listed block k: a gather, so it leaves no holes.  Unlisted blocks are empty (what d = 0 gives there).
 * P is clipped to the grid; the register holds bits only, no records, and is an ordinary operand of vc_hull_compare and
 * vc_hull_combine afterwards.  Stats (required): warped = |P|, common = |P & A|, a = |A|, warp_ms.  Refused as vc_hull_motion is,
 * for dst >= VC_HULL_REGISTERS, src == dst and a field made against another register.  A refused or failed call leaves dst as
 * it was.
 *
 * vc_paint_motion recolours every record by its block's vector, as vc_paint_clusters recolours: channel = 128 + (127 d_axis) / s
 * with C integer division, x -> R, y -> G, z -> B; index and seen byte stay.  A colour pass: it invalidates what colour passes
 * invalidate and nothing else.
 * vc_hull_motion is synchronous with one read-back in the middle (the number of listed blocks). */
typedef struct {
    uint32_t block;                     /* k */
    int8_t d[3];                        /* x, y, z */
    uint8_t flags;                      /* bit 0: clipped by the search range */
    uint32_t cost, cost0;
    uint16_t count_a, count_b, ties, reserved;
} vc_motion_t;
typedef struct {
    uint64_t blocks, listed, moved, unique, clipped, cost0_sum, cost_sum, a, b;
    float motion_ms;
} vc_motion_stats_t;
typedef struct {
    uint64_t warped, common, a;
    float warp_ms;
} vc_warp_stats_t;
int vc_hull_motion(vc_ctx *ctx, uint32_t reg, uint32_t block, uint32_t apron, uint32_t search, uint32_t flags /* must be 0 */,
                   vc_motion_stats_t *stats);
int vc_fetch_motion(vc_ctx *ctx, vc_motion_t *rows /* NULL ok */, uint64_t *count /* NULL ok */);
int vc_hull_warp(vc_ctx *ctx, uint32_t src, uint32_t dst, uint32_t flags /* must be 0 */, vc_warp_stats_t *stats);
int vc_paint_motion(vc_ctx *ctx);

/* ---- coarse-to-fine block motion: vectors beyond the search range (no reference counterpart) ---------------------------------------
 * vc_hull_motion finds no vector longer than s <= 8 voxels.  vc_hull_motion_pyramid is a second entry point to the same field:
 * it halves both hulls L times, matches the coarsest level as vc_hull_motion does, and on every finer level lets each block choose
 * among the displacements around twice its parent block's vector and twice the vectors of the parent's face neighbours.  Integers
 * and bits only (tests/motion_pyramid_np.py restates it bit for bit).  vc_hull_motion keeps its results.
 *   1 parameters: levels L in 0..3, refine radius r in 1..s; block, apron and search as for vc_hull_motion, refused in the same
 *     words (b + 2a + 2s <= 64 covers r).  reach = s 2^L + r (2^L - 1) <= 120 bounds every component of a vector, so int8 d holds
 *     it.  With L = 0, r is checked and otherwise unused: rows, vectors, counters and the nine stats of vc_motion_stats_t equal
 *     vc_hull_motion's bit for bit.
 *   2 levels: level 0 is the grid; level l has ceil(n / 2) cells per axis of level l - 1.  Cell v of A_l is the OR of the at most
 *     eight cells 2v + {0,1}^3 of A_{l-1} that lie in its grid; B_l likewise from the register's words.  Linear order and word
 *     layout are the same on every level: (iz nx_l + ix) ny_l + iy, 64 cells per word, the bits from n_l on zero.
 *     vc_fetch_motion_occupancy returns these words (which = 0: A, 1: B; level 0: the result's and the register's own).
 *   3 coarsest level: vc_hull_motion's items 1 to 4 applied to (A_L, B_L) with b, a and s, unchanged.
 *   4 listing and parents on a level l < L: blocks of edge b on level l's grid, listed when they hold a cell of A_l or of B_l, in
 *     ascending block index.  The parent of block (bx, by, bz) is block (bx >> 1, by >> 1, bz >> 1) of level l + 1.  With OR
 *     levels and an even b the parent of a listed block is listed; the device counts violations, and one is VC_ERR_HIP.
 *   5 candidates on a level l < L: the block's prediction is c = 2 d(parent); its centres are c and 2 d of each listed face
 *     neighbour of the parent (+-x, +-y, +-z in the coarser block grid), at most 7; its candidate set D is the union over the
 *     centres of centre + [-r, r]^3, a displacement reached from two centres counting once.
 *   6 choice on a level l < L: the cost of d in D is vc_hull_motion's on this level (the cells v of the window, the block grown by
 *     a, with A_l(v) != B_l(v - d); cells off the grid are empty).  The smallest (cost, |d - c|^2, dz, dx, dy) wins; ties = the
 *     distinct d in D at the smallest cost; cost0 = the cost of d = 0, whether or not 0 is in D.
 *   7 flags of a row of a level l < L: bit 0: some face neighbour d +- e_axis of the winner is not in D (a better vector may lie
 *     outside what was tried; on a single level this is vc_hull_motion's bit 0).  Bit 1: the winner does not lie in
 *     c + [-r, r]^3: it was borrowed from a neighbour's prediction.
 *   8 what the call leaves: the level-0 rows and vectors are the field: vc_fetch_motion, vc_hull_warp, vc_paint_motion and the
 *     lifetime of item 8 of vc_hull_motion apply unchanged, and vc_paint_motion divides by reach where it divides by s (with
 *     L = 0 the two are equal).  vc_fetch_motion_level returns the rows of level l <= L while the field is current (level 0:
 *     vc_fetch_motion's); a level above L, as `which` above 1, is VC_ERR_ARG.  A later vc_hull_motion leaves a field of L = 0.
 *   9 stats (required): the nine integers of vc_motion_stats_t over level 0; levels, refine, reach; listed_level[l] and
 *     dims_level[l] = (nx, ny, nz) of level l (0 above L); evaluated = the sum of |D| over the listed blocks of all levels
 *     below L; borrowed = the level-0 rows with bit 1; motion_ms.
 *  10 the call changes nothing: not the records, not the result generation, not the register.  Synchronous, one read-back per
 *     level (its listed blocks).  Refused as vc_hull_motion is (item 7 there), and for L > 3, r = 0, r > s. */
typedef struct {
    uint64_t blocks, listed, moved, unique, clipped, cost0_sum, cost_sum, a, b;
    uint32_t levels, refine, reach, reserved;
    uint64_t listed_level[4];
    uint32_t dims_level[4][3];
    uint64_t evaluated, borrowed;
    float motion_ms;
} vc_motion_pyramid_stats_t;
int vc_hull_motion_pyramid(vc_ctx *ctx, uint32_t reg, uint32_t block, uint32_t apron, uint32_t search, uint32_t levels, uint32_t refine,
                           uint32_t flags /* must be 0 */, vc_motion_pyramid_stats_t *stats);
int vc_fetch_motion_level(vc_ctx *ctx, uint32_t level, vc_motion_t *rows /* NULL ok */, uint64_t *count /* NULL ok */);
int vc_fetch_motion_occupancy(vc_ctx *ctx, uint32_t level, uint32_t which /* 0 = A, 1 = B */, uint64_t *words /* NULL ok */,
                              uint64_t *count /* NULL ok */);

/* ---- the vote over the last hulls, motion compensated (no reference counterpart) --------------------------------------------------
 * vc_hull_temporal never moves the older hulls, so on a figure that walks it votes the figure away: the hulls of five frames of a
 * body that moves two voxels a frame overlap in a sliver.  vc_hull_temporal_motion is a second entry point to the same ring and the
 * same P: before it counts, it aligns every older snapshot and P to the current hull by the block motion field between the ring's
 * newest snapshot and the current hull.  Integers and bits only (tests/temporal_motion_np.py restates it bit for bit).  Item
 * numbers in brackets are vc_hull_temporal's (T) and vc_hull_motion's (M) above.
 *   1 push, m, thresholds: as T1 - T3.  H_t is the current result's occupancy, m = min(pushes since the last reset, window), on
 *     and off scale with m.
 *   2 field: when the ring holds a hull before this push, F_t is the field of M1 - M4 with A = H_t and B = the ring's newest
 *     snapshot, which is the raw H_{t-1} (the newest snapshot is never moved before the next push), at block / apron / search
 *     with that call's ranges: b in {4, 8, 16}, a <= 16, 1 <= s <= 8, b + 2a + 2s <= 64, at most 2^26 blocks.  The first push after
 *     a reset has no field: listed = 0 and every motion stat but `blocks` is 0.
 *   3 align: for X = P and X = each snapshot that stays in the ring (the min(have, window - 1) newest, have = the hulls in the ring
 *     before this push): X'(v) = X(v - d_k) for v in listed block k; X'(v) = X(v) for v in an unlisted block (d = 0 there, NOT the
 *     emptying of vc_hull_warp: an old speck in a block that H_t and H_{t-1} both leave empty keeps its vote).  A source cell
 *     outside the grid is empty.  A gather: no holes.
 *   4 count and vote: c(v) counts over H_t and the aligned snapshots; O_t = { c >= on } + { v in P' : c >= off }.
 *   5 what the ring stores: the ALIGNED snapshots, and P becomes O_t.  The next call aligns them again by its own field, so a
 *     snapshot of age j has gone through a chain of j integer gathers.  What that costs: where neighbouring blocks have different
 *     vectors the content tears or doubles at the seam between them, such damage is never undone, and it compounds with age.
 *     vc_fetch_temporal_history(age) returns the aligned snapshot of that age; age 0 is the raw H_t.
 *   6 result, records, votes, `added`, invalidation: as T5.  A kept record keeps its 8 bytes, a voxel of O_t \ H_t is coloured as
 *     item 3 of vc_hull_grow colours one, and when O_t = H_t nothing is invalidated.  vc_fetch_temporal serves both calls.
 *   7 stats: window, frames, on, off, block, apron, search; survivors_before, survivors_after, added, removed; raw_changed =
 *     |H_t xor H_{t-1}| unaligned, as the plain call reports it; aligned_changed = |H_t xor H'_{t-1}|, what the field does not
 *     explain (0 when m = 1); out_changed = |O_t xor P'|; blocks, listed, moved, unique, clipped, cost0_sum, cost_sum as M5;
 *     temporal_ms = HIP events around the whole call.
 *   8 state and mixing: ring and P are vc_hull_temporal's, they survive what T7 says and are reset by what T7 says.  The ring
 *     remembers which of the two calls filled it: a call of the other kind starts it over, exactly as another `window` does.
 *     keep_on, keep_off, block, apron and search may change from call to call.  The field lives in a state of the call's own:
 *     a field of vc_hull_motion and the hull registers are neither read nor written.
 *   9 one push per result (T8), and VC_ERR_ARG by name, with nothing launched and no state touched, for everything T9 lists and
 *     for the parameters M7 refuses.
 *  10 a failure leaves result, ring and P as they were (T10): the aligned snapshots are written to a second ring beside the
 *     first (a gather cannot run in place anyway), O_t to the staging buffer, every buffer is sized before anything is
 *     committed, and the commit is a swap of the two rings.  The aligned P is used by the vote alone and is not stored.
 *  11 vc_fetch_temporal_motion: the rows of the call that produced the current result, as vc_fetch_motion returns rows; the count
 *     is 0 for a first push.  It fails when vc_fetch_temporal fails, and after a vc_hull_temporal.
 * Memory: (2 window + 2) nwords 8 bytes (1.6 GB at 1024^3 with window 5) and the field's few bytes per block.  Synchronous, two
 * read-backs: the listed blocks, then the counters.  What it does not do: everything vc_hull_motion does not do (no sub-voxel
 * vectors, no search beyond 8, no regularisation of the field), no per-snapshot fields that would avoid the accumulated warp,
 * and multi-GPU is refused. */
typedef struct {
    uint32_t window, frames /* m */, on, off, block, apron, search, reserved;
    uint64_t survivors_before, survivors_after, added, removed, raw_changed, aligned_changed, out_changed;
    uint64_t blocks, listed, moved, unique, clipped, cost0_sum, cost_sum;
    float temporal_ms;
} vc_temporal_motion_stats_t;
int vc_hull_temporal_motion(vc_ctx *ctx, uint32_t window, uint32_t keep_on, uint32_t keep_off, uint32_t block, uint32_t apron, uint32_t search,
                            uint32_t flags /* must be 0 */, vc_temporal_motion_stats_t *stats);
int vc_fetch_temporal_motion(vc_ctx *ctx, vc_motion_t *rows /* NULL ok */, uint64_t *count /* NULL ok */);

/* ---- ray-cast images of the current result (no reference counterpart: the reference's viewer draws instanced cubes with OpenGL,
 *      executable.py) -----------------------------------------------------------------------------------------------------------
 * vc_render casts one ray per pixel of each view through the current carve result and keeps, per pixel, the first survivor the
 * ray meets.  The result is read as vc_fetch_occupancy and vc_fetch_records see it, so it includes vc_color_visible,
 * vc_photo_carve and vc_hull_components.  The contract, bit for bit (tests/render_np.py restates it).  Everything is float64
 * with no contraction, evaluated in the order written:
 *   1 grid: every axis has n >= 2; along axis a, s = (max - min) / (n - 1), e = min - 0.5 * s, voxel boundary k is
 *     b(k) = e + (double)k * s, voxel c spans [b(c), b(c + 1)]; x <-> ix, y <-> iy, z <-> iz; i = (iz nx + ix) ny + iy.
 *   2 pixel ray of (u, v), 0 <= u < W, 0 <= v < H: xd = ((u + 0.5) - cx) / fx, yd = ((v + 0.5) - cy) / fy; x = xd, y = yd;
 *     then exactly 8 fixed-point undistortion steps, each from the previous x, y:
 *       r2 = x*x + y*y;  cd = ((1 + k1*r2) + (k2*r2)*r2) + ((k3*r2)*r2)*r2;
 *       dx = ((2*p1)*x)*y + p2*(r2 + (2*x)*x);  dy = p1*(r2 + (2*y)*y) + ((2*p2)*x)*y;  x, y = (xd - dx)/cd, (yd - dy)/cd.
 *     Direction d_j = (x*R[0][j] + y*R[1][j]) + R[2][j]; origin o_j = -((R[0][j]*t0 + R[1][j]*t1) + R[2][j]*t2) (element by
 *     element: the camera z of d is 1, so t below is the camera depth up to rounding).
 *   3 entry: for an axis with d_a != 0, inv_a = 1.0 / d_a and the slab parameters (b(0) - o_a) * inv_a, (b(n_a) - o_a) * inv_a;
 *     near_a is their min, far_a their max.  An axis with d_a == 0 (either sign) is a miss if o_a < b(0) or o_a >= b(n_a), else
 *     its near is -inf and its far +inf.  t_in = max(0, near_0, near_1, near_2), t_out = min(far); a miss if t_in >= t_out.
 *     If t_in > 0 the entry axis a* is the lowest axis with near_a == t_in, and its cell is 0 if d > 0, else n - 1.  Every other
 *     axis (all of them when t_in == 0) takes clamp(floor(((o_a + t_in * d_a) - e_a) / s_a), 0, n_a - 1).
 *   4 walk: a survivor cell is a hit at parameter t (t_in at first, then the t of the last step).  Otherwise each axis with
 *     d_a != 0 has its next boundary at tn_a = (b(c_a + (d_a > 0)) - o_a) * inv_a, an axis with d_a == 0 tn_a = +inf; the walk
 *     steps along the axis of the smallest tn (ties: the lowest axis), t = tn_a, c_a moves by +1 if d_a > 0 else -1; a c_a out
 *     of [0, n_a) is a miss.  At most nx + ny + nz steps.
 *   5 per pixel, on a hit: idx = the linear index; depth = (float)t; face = 2a + (d_a > 0 ? 0 : 1) for the axis a of the last
 *     step (or of entry), 6 when the walk starts inside a survivor; rgb_k = (rec_rgb_k * shade[face] + 127) / 255 in integers,
 *     rec_rgb = the RGB of the voxel's record.  On a miss: idx = 0xFFFFFFFF, depth = +inf, face = 255, rgb = background.
 * shade: u8 [7] per face (NULL = all 255); background: RGB (NULL = 0, 0, 0).  flags must be 0.  VC_ERR_ARG (with a message)
 * when there is no carve result, steps are in flight, the carve ran with VC_FLAG_NO_RECORDS, the slab is narrower than the grid,
 * a communicator of more than one rank is attached, a grid axis is shorter than 2, n_views == 0, H or W is outside 1..16384,
 * n_views * H * W > 2^28, a view parameter is not finite, fx <= 0 or fy <= 0, or flags != 0; a refused call leaves the images of
 * the last render as they were.  S = 0 is no error (every pixel a miss).  Synchronous.
 * The images stay valid until the next vc_render or vc_destroy; a new carve does not touch them.  vc_fetch_render copies one
 * view of them out ([H W] each, rgb [H W 3]; any pointer may be NULL); it fails before the first render and for view >= n_views.
 * stats (may be NULL): pixels = n_views H W, hits = pixels with a hit (both contract); cells_visited, blocks_skipped are
 * diagnostics of the walk the device took (option render_blocks); render_ms = HIP events around the whole call. */
typedef struct {
    double K[4];      /* fx, fy, cx, cy (no skew) */
    double dist[5];   /* k1, k2, p1, p2, k3; all zero = plain pinhole */
    double R[9];      /* world -> camera, row-major, as vc_set_cameras */
    double t[3];      /* mm */
} vc_view_t;
typedef struct {
    uint64_t pixels, hits;                    /* contract */
    uint64_t cells_visited, blocks_skipped;   /* diagnostics, implementation-defined */
    float render_ms;                          /* HIP events around the whole call */
} vc_render_stats_t;
int vc_render(vc_ctx *ctx, uint32_t n_views, const vc_view_t *views, uint32_t H, uint32_t W, const uint8_t *shade,
              const uint8_t *background, uint32_t flags, vc_render_stats_t *stats);
int vc_fetch_render(vc_ctx *ctx, uint32_t view, uint32_t *idx, float *depth, uint8_t *rgb, uint8_t *face);

/* ---- surface normals of the hull; smooth-shaded renders and mesh normals (no reference counterpart) -----------------------------
 * vc_hull_normals gives every surface record of the current carve result, as vc_fetch_occupancy and vc_fetch_records see it, the
 * direction its surface faces: minus the sum of the offsets to the survivors inside a ball in world units.  The contract, bit for
 * bit (tests/normals_np.py restates it).  Signed 64-bit integers only, and a sum over a set: the result does not depend on
 * evaluation order.
 *   1 input, metric: items 1 and 2 of vc_hull_distance, with the same refusals; q_a in um.
 *   2 ball: B(r2) = { (dx, dy, dz) != 0 : (q_x dx)^2 + (q_y dy)^2 + (q_z dz)^2 <= r2 }, r2 in um^2; ext_a = the largest k with
 *     (k q_a)^2 <= r2.  VC_ERR_ARG when B is empty or some ext_a > 15 (a voxel's y window then fits in 31 bits).
 *   3 surface: a record is SURFACE iff one of its 6 face neighbours is not a survivor or lies outside the grid (rule 1 of
 *     vc_color_visible's surface test).
 *   4 gradient of a surface record v: g(v) = sum over d in B with v + d inside the grid and ON of (q_x dx, q_y dy, q_z dz).  The
 *     border is open: outside the grid is OFF, nothing wraps around.  The normal is n = -g: from solid to empty, in world
 *     (x, y, z), in um-weighted units; |n_a| < 2^39.
 *   5 stored form, int16 [4] per record in record order: m = max |n_a|, n16_a = (n_a * 32767) / m truncated toward zero (C's /),
 *     w = 1.  A surface record with n = 0 stores (0, 0, 0, 1), a record that is not surface (0, 0, 0, 0).
 *   6 lifetime: the call leaves the result alone.  The normals stay valid across vc_color_visible (colours only) and fail to
 *     fetch after anything that changes which voxels survive: a carve, vc_photo_carve, vc_hull_components, vc_hull_morphology,
 *     a vc_hull_grow that adds something.
 *   7 VC_ERR_ARG (with a message, nothing launched) when there is no carve result, steps are in flight, the carve ran with
 *     VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached, flags != 0,
 *     stats == NULL, the metric is out of range or item 2 refuses.  S = 0 is no error.  Synchronous.
 * stats (required): survivors; surface = surface records; zero = surface records with n = 0; offsets = |B|; q; ext; normals_ms =
 * HIP events around the whole call.  vc_fetch_record_normals: int16 [S][4] in record order; with n4 == NULL it copies nothing and
 * only tells whether the normals are valid (VC_OK) or stale (VC_ERR_ARG).
 *
 * vc_shade_render shades the images of the last vc_render with the normals; it needs valid normals and a render that ran on the
 * current result (a render made before a carve or a pass of item 6 is refused).  vc_fetch_render and its images are untouched.
 * Per pixel, idx from the render: a miss keeps the render's background.  A hit's record is the first with index >= idx (binary
 * search, as the render finds it); if its w = 0 or n16 = 0 the pixel keeps the render's own rgb.  Otherwise, in float64 with no
 * contraction and in this order, L = light[view] (from the surface towards the light, world coordinates):
 *     dot = ((double)n0*L0 + (double)n1*L1) + (double)n2*L2;  nn = (double)(n0*n0 + n1*n1 + n2*n2) (the integer is exact);
 *     ll = (L0*L0 + L1*L1) + L2*L2;  c = dot > 0 ? min(dot / sqrt(nn * ll), 1.0) : 0.0;
 *     s = ambient + (uint32_t)floor((double)(255 - ambient) * c + 0.5);  rgb_k = (rec_rgb_k * s + 127) / 255 in integers,
 * rec_rgb = the record's RGB as it is at this call.  VC_ERR_ARG when a light component is not finite, ll is not a finite normal
 * number, ambient > 255, flags != 0, the normals are stale, or the render is stale or missing.  vc_fetch_shaded: rgb [H W 3] of
 * one view; fails before the first vc_shade_render on the last render and for view >= n_views.
 *
 * vc_surface_normals: per vertex of the last vc_surface_mesh, the stored quadruple of the ON element's record (the vertex's edge
 * entry holds the element; same search), int16 [V][4].  VC_ERR_ARG unless the mesh was made on the current result and the
 * normals are valid. */
typedef struct {
    uint64_t survivors, surface, zero /* surface records with n = 0 */, offsets /* |B| */;
    uint64_t q[3];                  /* x, y, z in um */
    uint32_t ext[3];
    float normals_ms;               /* HIP events around the whole call */
} vc_normals_stats_t;
int vc_hull_normals(vc_ctx *ctx, uint64_t r2, uint32_t flags /* must be 0 */, vc_normals_stats_t *stats);
int vc_fetch_record_normals(vc_ctx *ctx, int16_t *n4);             /* [S][4], record order */
int vc_shade_render(vc_ctx *ctx, const double *light /* [n_views][3] */, uint32_t ambient /* 0..255 */, uint32_t flags /* must be 0 */);
int vc_fetch_shaded(vc_ctx *ctx, uint32_t view, uint8_t *rgb);     /* [H W 3] */
int vc_surface_normals(vc_ctx *ctx, int16_t *n4);                  /* [V][4], vertex order of vc_fetch_surface_mesh */

/* ---- free-viewpoint images: sub-voxel ray hits textured from the camera frames (no reference counterpart) -------------------------
 * vc_texture_render is a pass over the images of the last vc_render, like vc_shade_render: every hit is refined along its own ray
 * against the silhouettes, and the pixel is coloured from the cameras that see the refined point, weighted by how close they look
 * to the viewing direction.  It reads the render's images, the current carve result's cameras, masks and threshold, the depth maps
 * of a current vc_color_visible and the images of frame set `slot` (every camera needs one); it changes none of them, and
 * vc_fetch_render, vc_fetch_shaded and the records stay as they are.  The contract, bit for bit (tests/texture_np.py restates it);
 * float64 with no contraction, in the order written, unless stated otherwise.  Per pixel of each view of the last render; a miss
 * keeps the render's pixel:
 *   1 ray: o, d = item 2 of vc_render for the stored view; t0 = (double)depth of the render; P(t)_j = o_j + t * d_j (one multiply,
 *     one add).
 *   2 inside(P) = item 2 of vc_surface_mesh: the carve's cameras, the post-filtered masks the carve read, T(P) >= m.
 *   3 refinement, steps in 0..24, reach_mm = L >= 0.  With steps > 0: in0 = inside(P(t0)); (lo, hi) = in0 ? (max(t0 - L, 0), t0) :
 *     (t0, t0 + L); the pixel is REFINED iff !inside(P(lo)) && inside(P(hi)); then `steps` times mid = (lo + hi) * 0.5,
 *     inside(P(mid)) ? hi = mid : lo = mid, and t = (lo + hi) * 0.5.  Otherwise (steps = 0, L = 0, the view inside the hull, or
 *     an occupancy that disagrees with the point test: a photo carve, a foreign lookup table) t = t0.  Output depth = (float)t.
 *   4 candidates, P = P(t): camera c of the carve with d_c = camera z of P (item 3 of vc_color_visible) and (u, v) = the carve's
 *     projection of P is a candidate iff d_c > 0, 0 <= v < H_c and 0 <= u < W_c on the floats, and (float)d_c <=
 *     zmap_c[int(v) W_c + int(u)] + tol (the add in float32), zmap_c = the current vc_color_visible map of c, tol = depth_tolerance.
 *   5 weight of a candidate: C_c,j = -((R[0][j]*t0 + R[1][j]*t1) + R[2][j]*t2) from camera c's R and t (as item 2 of vc_render
 *     makes o); a = C_c - P, b = o - P; dot = (a0*b0 + a1*b1) + a2*b2, aa and bb alike; c = (dot > 0 and aa * bb is a finite
 *     normal number) ? min(dot / sqrt(aa * bb), 1.0) : 0.0; then `sharpen` times (0..6) c = c * c; w_c = (uint32_t)floor(c * 65535.0
 *     + 0.5).  A camera that is no candidate has w_c = 0.  Only the `best` (1..16) largest weights stay, ties to the lower camera
 *     index; the others count as 0.
 *   6 sample of camera c's image of `slot`, read as RGB.  filter = 0: pixel int(v) W_c + int(u).  filter = 1, bilinear in integers:
 *     fu = u - 0.5, x0 = floor(fu), ax = (int)floor((fu - x0) * 256.0); fv, y0, ay alike; columns x0, x0 + 1 and rows y0, y0 + 1
 *     clamped into the image; per channel ch = ((p00 (256 - ax) + p10 ax)(256 - ay) + (p01 (256 - ax) + p11 ax) ay + 32768) >> 16,
 *     p10 = the pixel at column x0 + 1 of row y0, p01 = column x0 of row y0 + 1.
 *   7 blend: Ws = sum of the w_c that stayed.  Ws == 0: the pixel keeps the render's rgb, count = 0, best_cam = 255.  Otherwise per
 *     channel ch = (sum w_c ch_c + Ws / 2) / Ws in 64-bit integers, count = the cameras with w_c > 0 that stayed, best_cam = the
 *     heaviest of them.  A miss has count = 0, best_cam = 255, refined = 0 and depth +inf.
 * stats (required): pixels = n_views H W, hits, refined, textured = hits with Ws > 0, fallback = hits with Ws == 0 (all contract);
 * point_tests = camera tests of item 2 the device evaluated (a diagnostic: it stops a point's test once it is decided);
 * texture_ms = HIP events around the whole call.  VC_ERR_ARG (with a message, nothing launched, the textured images of an
 * earlier call left as they were) when there is no carve result, steps are in flight, the carve ran with VC_FLAG_NO_RECORDS, the
 * slab is narrower than the grid, a communicator of more than one rank is attached, the last render is missing or did not run on
 * the current result, vc_color_visible has not run on the current result, a camera of `slot` has no image, steps > 24, best
 * outside 1..16, sharpen > 6, filter > 1, reach_mm or depth_tolerance negative or not finite, flags != 0, stats == NULL, or --
 * with steps > 0 -- the carve's frame set has been prepared again since the carve or has new masks or images waiting for it
 * (vc_surface_mesh's rule).  An empty hull is no error.  Synchronous.
 * The images stay valid until the next vc_texture_render, the next vc_render or vc_destroy.  vc_fetch_textured copies one view
 * out (rgb [H W 3], the others [H W]; any pointer may be NULL); it fails before the first vc_texture_render on the last render
 * and for view >= n_views. */
typedef struct {
    uint64_t pixels, hits, refined, textured, fallback;   /* contract: textured + fallback = hits */
    uint64_t point_tests;                                 /* diagnostic, implementation-defined */
    float texture_ms;                                     /* HIP events around the whole call */
} vc_texture_stats_t;
int vc_texture_render(vc_ctx *ctx, uint32_t slot, uint32_t steps, double reach_mm, float depth_tolerance, uint32_t best,
                      uint32_t sharpen, uint32_t filter, uint32_t flags /* must be 0 */, vc_texture_stats_t *stats);
int vc_fetch_textured(vc_ctx *ctx, uint32_t view, uint8_t *rgb, float *depth, uint8_t *count, uint8_t *best_cam, uint8_t *refined);

/* ---- lit renders: cast shadows, ambient occlusion and a floor (the reference's viewer has a positioned light, a shadow map and a
 * floor grid; this is their headless counterpart, not a port) ------------------------------------------------------------------------
 * vc_light_render is a pass over the images of the last vc_render, like vc_shade_render and vc_texture_render: every hit pixel,
 * and every pixel that sees the floor, casts one ray to the light and sixteen rays into the hemisphere above its face through the
 * current carve result.  It reads the render's images, the occupancy, the records and -- with smooth = 1 -- the normals of a
 * current vc_hull_normals; it changes none of them, and vc_fetch_render, vc_fetch_shaded and vc_fetch_textured stay as they are.
 * The contract, bit for bit (tests/light_np.py restates it); float64 with no contraction, in the order written.  Symbols are
 * those of items 1-5 of vc_render.  Per pixel of each view of the last render:
 *   1 primary ray and point: o, d = item 2 of vc_render for the stored view.  A HULL pixel is a hit of the render that is no
 *     floor pixel; t' = (double)depth of the render, Q_a = o_a + t' * d_a.
 *   2 start cell: c = the hit cell (from idx), face = 2a + k.  c0 = c moved one cell along axis a, by -1 when k = 0 and by +1 when
 *     k = 1: the cell the primary ray came from, empty or outside the grid.  The outward sign is sigma = -1 for k = 0, +1 for
 *     k = 1.  Face 6 (the camera inside a survivor): the pixel keeps the render's rgb, shadow = 0, ao = 16, and casts no ray.
 *     c0 outside the grid: every secondary ray of the pixel is open (it leaves a convex grid).
 *   3 secondary walk: item 4 of vc_render from cell c0 with t = 0, origin Q and a direction e -- the same tn, the same tie rule,
 *     the same step bound; it starts from the given cell, not from item 3's entry, so that rounding of Q cannot put the ray back
 *     into the voxel it left.  It gives hit or miss and the hit's t.
 *   4 shadow ray: e = pos[0..2] - Q for a point light (pos[3] = 1, world mm), pos[0..2] for a directional one (pos[3] = 0, from
 *     the surface towards the light).  sigma * e_a <= 0: the face is turned away, shadow = 2, no walk.  Otherwise the ray is
 *     occluded iff the walk hits and, for a point light, t < 1; shadow = 1 when occluded, else 0.
 *   5 occlusion rays: sixteen vectors (iu, iv, in) in the face's frame, u = (a + 1) % 3, v = (a + 2) % 3, the normal axis a with
 *     sign sigma.  Four rings of four: (+-1, 0, 2) and (0, +-1, 2); (+-1, +-1, 2); (+-1, 0, 1) and (0, +-1, 1); (+-1, +-1, 1); in a
 *     ring the order is +u, -u, +v, -v, or (+, +), (+, -), (-, +), (-, -).  e_u = (double)iu * s_u, e_v = (double)iv * s_v,
 *     e_a = (double)(sigma in) * s_a.  Ray k is occluded iff its walk hits with t < ao_reach / sqrt((double)(iu^2 + iv^2 + in^2)).
 *     ao = the open rays, 0..16; ao_reach = 0: no rays, ao = 16.
 *   6 floor (floor = 1): a FLOOR pixel has d_z != 0, tf = (floor_z - o_z) / d_z > 0, is a miss of the render or has
 *     tf < (double)depth, and Q = o + tf * d has floor_rect[0] <= Q_x <= floor_rect[1], floor_rect[2] <= Q_y <= floor_rect[3].
 *     Its base colour is floor_rgb[(kx + ky) & 1], kx = (int64)floor(Q_x / floor_cell_mm), ky alike.  Its frame is a = 2,
 *     sigma = -1 if o_z < floor_z, else +1.  Its secondary rays are items 3 AND 4 of vc_render in full (entry, then walk) from
 *     origin Q -- the floor may lie outside the grid --, judged by 4 and 5 above; a ray that misses the grid is open.
 *   7 shade: the normal is the record's of vc_hull_normals when smooth = 1, its w = 1 (w is 0 or 1: any w != 0 counts) and n16 != 0,
 *     else the face normal (sigma on
 *     axis a, 0 elsewhere); always the face normal on the floor.  c as in vc_shade_render with L = e of the shadow ray.
 *     a_term = (ambient * ao * 2 + 16) / 32 in integers; s = a_term + (shadow ? 0 : (uint32_t)floor((double)(255 - ambient) * c +
 *     0.5)); rgb_k = (base_k * s + 127) / 255, base = the record's RGB as it is at this call, or the floor's colour.
 *   8 outputs: rgb; depth = the render's, (float)tf on the floor; kind = 0 background, 1 hull, 2 floor; shadow; ao.  A background
 *     pixel keeps the render's rgb and depth, shadow = 0, ao = 16.
 * stats (required): pixels = n_views H W, hull_pixels, floor_pixels, shadowed (shadow = 1), facing_away (shadow = 2), rays_walked =
 * the shadow rays of item 4 that are not turned away plus, when ao_reach > 0, 16 per hull or floor pixel -- face-6 pixels cast and
 * count none, an open ray of a start cell outside the grid counts (all contract); cells_visited, blocks_skipped = diagnostics of
 * the walk the device took (option render_blocks, same images); light_ms = HIP events around the whole call.
 * VC_ERR_ARG (with a message, nothing launched, the lit images of an earlier call left as they were) when there is no carve
 * result, steps are in flight, the carve ran with VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more
 * than one rank is attached, the last render is missing or did not run on the current result, smooth = 1 without normals of the
 * current result, flags != 0, stats or light == NULL, a parameter that is not finite, pos[3] neither 0 nor 1, a direction whose
 * squared length is no normal number, ambient > 255, smooth or floor > 1, ao_reach < 0, and with floor = 1 an empty rectangle, or
 * floor_cell_mm not > 0 or so small that a bound of the rectangle is 2^52 cells or more from 0.  An empty hull is no error.
 * Synchronous.  The images stay valid until the next vc_light_render, the next vc_render or vc_destroy.  vc_fetch_lit copies one
 * view out (rgb [H W 3], the others [H W]; any pointer may be NULL); it fails before the first vc_light_render on the last render
 * and for view >= n_views. */
typedef struct {
    double pos[4];               /* x, y, z, w: w = 1 a point in world mm, w = 0 a direction from the surface towards the light */
    uint32_t ambient;            /* 0..255 */
    uint32_t smooth;             /* 1: shade by the normals of vc_hull_normals */
    double ao_reach;             /* >= 0, in grid steps (the comparison of item 5); 0: no occlusion rays */
    uint32_t floor;              /* 0 | 1 */
    double floor_z;
    double floor_rect[4];        /* x0, x1, y0, y1 */
    double floor_cell_mm;        /* > 0 */
    uint8_t floor_rgb[2][3];
} vc_light_t;
typedef struct {
    uint64_t pixels, hull_pixels, floor_pixels, shadowed, facing_away, rays_walked;   /* contract */
    uint64_t cells_visited, blocks_skipped;                                            /* diagnostics, implementation-defined */
    float light_ms;                                                                    /* HIP events around the whole call */
} vc_light_stats_t;
int vc_light_render(vc_ctx *ctx, const vc_light_t *light, uint32_t flags /* must be 0 */, vc_light_stats_t *stats);
int vc_fetch_lit(vc_ctx *ctx, uint32_t view, uint8_t *rgb, float *depth, uint8_t *kind, uint8_t *shadow, uint8_t *ao);

/* ---- the hull split into K figures on the floor plane (no reference counterpart) --------------------------------------------------
 * vc_hull_clusters runs K-means over the columns of the current carve result, as vc_fetch_occupancy and vc_fetch_records see it
 * (photo carve, components, morphology, grow and footprint rules included): world "up" is -z, so a floor position is a column
 * (ix, iy).  The result is left exactly as it is.  The contract, bit for bit (tests/clusters_np.py restates it).  Integers only, and
 * every sum is a sum over a set: the outputs do not depend on evaluation order.
 *   inputs: K in 1..16; max_iters in 1..255; min_column (0 and 1: no floor); hist_iz_lo <= hist_iz_hi < nz, the inclusive band of
 *     layers of the colour signature; init NULL or int64 [K][2], centres in um from the grid's (x_min, y_min) corner, every
 *     component within +-2^30 (d2 then fits int64); flags = 0; stats (required).
 *   1 metric: q_x, q_y = item 2 of vc_hull_distance for the x and y axes only, llrint(((max - min) / (n - 1)) * 1000.0) with that
 *     item's refusals for those two axes.  Column (ix, iy) has index col = ix ny + iy and position P = (q_x ix, q_y iy);
 *     d2(P, c) = (P_x - c_x)^2 + (P_y - c_y)^2 in int64.
 *   2 floor map: n[col] = the number of survivors i with i mod (nx ny) = col (u32); weight w = n if n >= min_column, else 0;
 *     Wtot = sum w.  With Wtot = 0 (S = 0, for example) there are no rounds: iterations = 0, converged = 1, every label is 0, the
 *     centres are init, or zeros.
 *   3 seeding when init is NULL: M = ((sum w P_x + Wtot / 2) div Wtot, the same for y); c_0 = the position of the weighted column
 *     (w > 0) with the smallest d2(P, M); for j = 1 .. K - 1, c_j = the position of the weighted column that maximises
 *     min_{i<j} d2(P, c_i) (farthest first).  Every tie goes to the lowest col.  Fewer weighted columns than K give duplicate
 *     centres, and the duplicates end up empty under item 4.
 *   4 round r = 1, 2, ...: every column with n > 0 takes label = argmin_k d2(P, c_k), a tie the lowest k; then every k with
 *     W_k = sum over label = k of w > 0 takes c_k = ((sum w P_x + W_k / 2) div W_k, the same for y); a cluster with W_k = 0 keeps
 *     its centre.  The rounds stop after the one in which no centre changed (converged = 1, iterations = r), else after
 *     max_iters (converged = 0).  Every sum stays below 2^62.
 *   5 outputs.  vc_fetch_cluster_labels: u8 [S], each record its column's label of the last round.  vc_fetch_clusters:
 *     vc_cluster_t [K] -- centre_um; voxels = the records with that label; weight = W_k of the last round; columns = the columns
 *     with n > 0 and that label; lo / hi = the inclusive box of its records in (ix, iy, iz), and lo = 0xffffffff, hi = 0 on every
 *     axis (lo > hi) for a cluster without a record.  vc_fetch_cluster_histograms: u32 [K][512], bin (r >> 5) << 6 | (g >> 5) << 3
 *     | (b >> 5) over the records of label k whose seen byte is 1 and whose iz lies in the band, with the colours the records have
 *     at the call.  vc_fetch_floor_map: u32 [nx ny], n.  vc_fetch_floor_labels: u8 [nx ny], 255 where n = 0.
 *   6 vc_paint_clusters(rgb u8 [K][3]): every record's RGB becomes its label's entry; index and seen byte stay, as
 *     vc_color_visible recolours in place.  The next carve gives the camera colours again.
 *   7 VC_ERR_ARG (with a message, nothing launched) when there is no carve result, steps are in flight, the carve ran with
 *     VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached, K, max_iters, the
 *     band, init or the metric is out of range, flags != 0, stats == NULL.  S = 0 is no error.  Synchronous.
 *   8 lifetime: the fetch calls and vc_paint_clusters fail until the pass has run on the current result and again after anything
 *     that changes which voxels survive (a carve, vc_photo_carve, vc_hull_components, vc_hull_morphology, a vc_hull_grow that adds
 *     something), as vc_fetch_component_labels does; colour passes (vc_color_visible, vc_paint_clusters) leave them valid.
 * stats (required): survivors; columns = columns with n > 0; weight = Wtot; iterations; converged; q; clusters_ms = HIP events
 * around the whole call. */
typedef struct {
    int64_t centre_um[2];
    uint64_t voxels, weight;
    uint32_t columns, lo[3], hi[3];
} vc_cluster_t;
typedef struct {
    uint64_t survivors, columns, weight;
    uint64_t q[2];                  /* x, y in um */
    uint32_t iterations, converged;
    float clusters_ms;              /* HIP events around the whole call */
} vc_cluster_stats_t;
int vc_hull_clusters(vc_ctx *ctx, uint32_t K, uint32_t max_iters, uint32_t min_column, uint32_t hist_iz_lo, uint32_t hist_iz_hi,
                     const int64_t *init /* [K][2] um, or NULL */, uint32_t flags /* must be 0 */, vc_cluster_stats_t *stats);
int vc_fetch_cluster_labels(vc_ctx *ctx, uint8_t *labels);                 /* [S], record order */
int vc_fetch_clusters(vc_ctx *ctx, vc_cluster_t *out);                     /* [K] */
int vc_fetch_cluster_histograms(vc_ctx *ctx, uint32_t *hist);              /* [K][512] */
int vc_fetch_floor_map(vc_ctx *ctx, uint32_t *n);                          /* [nx ny] */
int vc_fetch_floor_labels(vc_ctx *ctx, uint8_t *labels);                   /* [nx ny] */
int vc_paint_clusters(vc_ctx *ctx, const uint8_t *rgb /* [K][3] */);

/* ---- geodesic distances through the hull, its extremities, their regions and paths (no reference counterpart) ---------------------
 * vc_hull_geodesic measures every survivor's distance to a seed set along paths that stay inside the current carve result, as
 * vc_fetch_occupancy and vc_fetch_records see it, then picks K extremities by repeated farthest-point selection: head, hands,
 * feet.  The result is left exactly as it is.  The contract, bit for bit (tests/geodesic_np.py restates it).  Integers only.
 *   1 graph: the nodes are the survivors; an edge joins two survivors that are `connectivity`-neighbours (6, 18 or 26: offsets
 *     (dx, dy, dz) in {-1, 0, 1}^3 with 1, up to 2 or up to 3 non-zero components, as in vc_hull_components).  With q_x, q_y, q_z =
 *     item 2 of vc_hull_distance (its refusals included), the edge of offset (dx, dy, dz) has length w = (isqrt(4 s) + 1) div 2 um,
 *     s = (q_x dx)^2 + (q_y dy)^2 + (q_z dz)^2: the Euclidean length rounded to the nearest um.  The 7 lengths are computed on the
 *     host; stats.edge_um[m - 1] is that of m = |dx| | |dy| << 1 | |dz| << 2.
 *   2 sources and keys: the seed set is source 0.  Every voxel has a key (d, label), compared lexicographically: the minimum over
 *     all paths from any source of (path length in um as u64, that source's label).  Nothing saturates (S w < 2^53).  An unreached
 *     voxel has (2^64 - 1, 255).  Packed, a key is d << 8 | label, and relaxing key(v) = min(key(v), key(u) + (w << 8)) over the
 *     edges reaches this fixpoint from any schedule and from any start whose keys are lengths of real paths.
 *     seed_mode VC_GEO_SEEDS_LIST: seeds = n_seeds linear indices (duplicates allowed; n_seeds = 0 seeds nothing; `layers` is
 *     ignored).  VC_GEO_SEEDS_IZ_MAX: every survivor of the layers iz_max - layers + 1 .. iz_max, iz_max = the highest layer that
 *     holds a survivor (world "up" is -z: the floor contact); VC_GEO_SEEDS_IZ_MIN: of iz_min .. iz_min + layers - 1 (the top);
 *     layers >= 1, `seeds` is ignored.  stats.seeds = the distinct seed voxels.
 *   3 extremities, for k = 1 .. K (K <= VC_GEO_MAX_K): E_k = the reached voxel with the largest d, a tie the lowest linear index;
 *     the selection stops when that d is 0 (or nothing is reached).  vc_extremum_t records (d, voxel, record, ix, iy, iz, label =
 *     k).  E_k then becomes the source of label k (its key is (0, k)) and the relaxation goes on from the keys as they are.  After
 *     the last one label(v) is the region of v and d(v) the distance to its nearest source.  stats.extremities = how many were found.
 *   4 paths: next(v) = the lowest-index neighbour u with key(u) + (w << 8) == key(v).  Following next from any reached voxel ends
 *     at a voxel with d = 0; the path is the list of linear indices, v first.  vc_geodesic_path walks it through the final keys
 *     (from an extremity that is just that voxel: it is a source).  With VC_GEO_PATHS in flags, the path of every E_k is walked
 *     when E_k is picked, before it becomes a source -- back to the nearest of the seed set and E_1 .. E_(k-1): the stick figure;
 *     vc_fetch_extremum_path(k) returns it.
 *   5 vc_paint_geodesic(mode, palette): every record's RGB becomes palette[label] (mode VC_GEO_PAINT_LABELS; palette u8
 *     [VC_GEO_MAX_K + 1][3]) or the grey 255 d div max_d (mode VC_GEO_PAINT_DISTANCE, max_d = stats.max_d, grey 0 when it is 0; the
 *     palette may be NULL); an unreached voxel takes VC_GEO_UNREACHED_R / _G / _B in both.  Index and seen byte stay, as
 *     vc_paint_clusters recolours in place; the next carve gives the camera colours again.
 *   6 VC_ERR_ARG (with a message, nothing launched that changes an output) when there is no carve result, steps are in flight,
 *     the carve ran with VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached,
 *     flags has a bit other than VC_GEO_PATHS, stats == NULL, connectivity is not 6, 18 or 26, K > VC_GEO_MAX_K, seed_mode is
 *     unknown, layers = 0 with a layer mode, seeds == NULL with n_seeds > 0, the metric is out of range, or a seed is no survivor
 *     (the message names the first such seed and its voxel).  S = 0 is no error.  Synchronous.  VC_ERR_INTERNAL when a relaxation
 *     has not settled after S + 1 launches of its rounds (it cannot: every round but the last lowers a key).
 *   7 lifetime: the fetch calls, vc_geodesic_path and vc_paint_geodesic fail until the pass has run on the current result and
 *     again after anything that changes which voxels survive, as vc_fetch_component_labels does; colour passes (vc_color_visible,
 *     vc_paint_clusters, vc_paint_geodesic) leave them valid.
 * Two routes relax, with equal bytes: tiles of VC_GEO_TILE_X x _Y x _Z cells laid from the low corner of the survivors' index box,
 * one workgroup per listed tile and launch (option geodesic_tiles = 1), or sweeps of one lane per record over the whole hull
 * (geodesic_tiles = 0).  stats: survivors, seeds, reached, unreached, max_d (the largest d of a reached voxel after the last
 * relaxation), tile_visits (tiles taken by a workgroup, summed over the launches; 0 on the sweep route), tiles (of the box),
 * extremities, rounds (tile route: launches of a tile list; sweep route: read-backs of the change flag), launches (relaxation
 * kernels launched), edge_um, q, geodesic_ms = HIP events around the whole call. */
#define VC_GEO_SEEDS_LIST   0u
#define VC_GEO_SEEDS_IZ_MAX 1u
#define VC_GEO_SEEDS_IZ_MIN 2u
#define VC_GEO_PATHS 1u
#define VC_GEO_MAX_K 32
#define VC_GEO_TILE_X 4
#define VC_GEO_TILE_Y 64
#define VC_GEO_TILE_Z 4
#define VC_GEO_PAINT_LABELS   0u
#define VC_GEO_PAINT_DISTANCE 1u
#define VC_GEO_UNREACHED_R 255
#define VC_GEO_UNREACHED_G 0
#define VC_GEO_UNREACHED_B 255
typedef struct {
    uint64_t d;                     /* um, at the moment it was picked */
    uint32_t voxel, record, ix, iy, iz, label;
} vc_extremum_t;
typedef struct {
    uint64_t survivors, seeds, reached, unreached, max_d, tile_visits, tiles;
    uint64_t edge_um[7];
    uint64_t q[3];
    uint32_t extremities, rounds, launches;
    float geodesic_ms;              /* HIP events around the whole call */
} vc_geodesic_stats_t;
int vc_hull_geodesic(vc_ctx *ctx, uint32_t connectivity, uint32_t seed_mode, const uint32_t *seeds, uint64_t n_seeds, uint32_t layers,
                     uint32_t K, uint32_t flags /* 0 or VC_GEO_PATHS */, vc_geodesic_stats_t *stats);
int vc_fetch_geodesic(vc_ctx *ctx, uint64_t *d);                           /* [S] um, 2^64 - 1 where unreached */
int vc_fetch_geodesic_labels(vc_ctx *ctx, uint8_t *labels);                /* [S], 255 where unreached */
int vc_fetch_extrema(vc_ctx *ctx, vc_extremum_t *out);                     /* [stats.extremities] */
int vc_geodesic_path(vc_ctx *ctx, uint32_t voxel, uint32_t *out, uint32_t capacity, uint32_t *n);
int vc_fetch_extremum_path(vc_ctx *ctx, uint32_t k /* 1 .. extremities */, uint32_t *out, uint32_t capacity, uint32_t *n);
int vc_paint_geodesic(vc_ctx *ctx, uint32_t mode, const uint8_t *palette /* [VC_GEO_MAX_K + 1][3] */);

/* ---- the hull's figures measured: volume, area, centroid, axes, per group of records (no reference counterpart) -------------------
 * vc_hull_measure reduces the records of the current carve result, as vc_fetch_occupancy and vc_fetch_records see it, to a few
 * integers per group.  The result is left exactly as it is.  The contract, bit for bit (tests/measure_np.py restates it).  Integers
 * only, and every value is a sum or an extremum over a set: neither evaluation order nor the arrival order of atomics shows.
 *   1 inputs: the S records in ascending linear index i = (iz nx + ix) ny + iy, each {u32 i, u8 r, g, b, seen}; the occupancy;
 *     a label per record from `source`:
 *       VC_MEASURE_ALL       one group, G = 1 (`labels` and `groups` are ignored);
 *       VC_MEASURE_CLUSTERS  the u8 labels of a vc_hull_clusters that is current, G = its K;
 *       VC_MEASURE_GEODESIC  the u8 region labels of a vc_hull_geodesic that is current, G = its extremities + 1; label 255
 *                            (unreached) belongs to no group;
 *       VC_MEASURE_HOST      labels = const uint32_t [S] in record order and G = groups; 0xffffffff belongs to no group.
 *     1 <= G <= VC_MEASURE_MAX_GROUPS.  Every axis of the grid has at most 65 536 cells: every sum then stays below 2^64.
 *   2 per group g, over its records, a vc_measure_t of 21 u64 followed by 6 u32, 192 bytes:
 *       voxels    its records                        surface   those with at least one exposed face
 *       seen      those whose seen byte is 1         s1[3]     sum ix, sum iy, sum iz
 *       s2[6]     sum ix^2, iy^2, iz^2, ix iy, ix iz, iy iz, in this order
 *       faces[6]  exposed faces towards -x, +x, -y, +y, -z, +z
 *       rgb[3]    sum r, sum g, sum b over the records with seen = 1, with the colours the records have at the call
 *       lo[3], hi[3]  the inclusive box in (ix, iy, iz); lo = 0xffffffff > hi = 0 on every axis for a group without a record,
 *                 as in vc_cluster_t.
 *     A face is exposed when the neighbour in that direction lies outside the grid or is no survivor of the whole hull, in
 *     whatever group it may be.  Nothing wraps around: i and i + 1 are no neighbours when (i + 1) mod ny = 0.
 *   3 VC_MEASURE_PROFILE in flags: besides, per group and layer iz, {n, sum ix, sum iy} over the group's records of that layer,
 *     u64 [G][nz][3] -- the cross-section and its centre line by height.  Refused when G nz > 2^20.
 *   4 VC_ERR_ARG (with a message, nothing launched) when there is no carve result, steps are in flight, the carve ran with
 *     VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached, source or a bit
 *     of flags is unknown, stats == NULL, an axis has more than 65 536 cells, the cluster or geodesic pass the source names is
 *     not current, labels == NULL with VC_MEASURE_HOST, G is out of range, or a host label is >= G and not 0xffffffff (the
 *     message names the first such record).  S = 0 is no error: every group is empty.  Synchronous.
 *   5 lifetime: vc_fetch_measure and vc_fetch_measure_profile fail ("no measurements") until the pass has run on the current
 *     result and again after anything that changes which voxels survive, as vc_fetch_component_labels does; the profile also
 *     when the last call ran without VC_MEASURE_PROFILE.  Colour passes leave them valid: the colour sums describe the records
 *     as they were at the call.  So does a later vc_hull_clusters or vc_hull_geodesic: the groups stay those of the labels that
 *     were current at the call, whatever the label source holds by now.  A vc_hull_grow or vc_hull_temporal that adds and
 *     removes nothing leaves them valid as well; one that changes the hull does not.
 * stats (required): survivors; groups = G; measured = the records in some group; unlabelled = survivors - measured;
 * measure_ms = HIP events around the whole call.  voxcarve.measure derives world units (mm^3, mm^2, centroid, principal axes)
 * from these integers and the grid on the host. */
#define VC_MEASURE_ALL      0u
#define VC_MEASURE_CLUSTERS 1u
#define VC_MEASURE_GEODESIC 2u
#define VC_MEASURE_HOST     3u
#define VC_MEASURE_PROFILE  1u
#define VC_MEASURE_MAX_GROUPS 4096u
#define VC_MEASURE_MAX_AXIS 65536u
#define VC_MEASURE_MAX_PROFILE (1u << 20)
typedef struct {
    uint64_t voxels, surface, seen;
    uint64_t s1[3], s2[6], faces[6], rgb[3];
    uint32_t lo[3], hi[3];
} vc_measure_t;
typedef struct {
    uint64_t survivors, measured, unlabelled;
    uint32_t groups;
    float measure_ms;               /* HIP events around the whole call */
} vc_measure_stats_t;
int vc_hull_measure(vc_ctx *ctx, uint32_t source, const uint32_t *labels /* [S], VC_MEASURE_HOST only */, uint32_t groups, uint32_t flags,
                    vc_measure_stats_t *stats);
int vc_fetch_measure(vc_ctx *ctx, vc_measure_t *out);                      /* [G] */
int vc_fetch_measure_profile(vc_ctx *ctx, uint64_t *out);                  /* [G][nz][3] */

/* ---- the hull's shell: what a viewer of opaque cubes can see, with faces and levels of detail (no reference counterpart) ----------
 * vc_hull_shell lists the cells of the current carve result that have an exposed face, in cell order, with their exposed faces,
 * at the voxels' resolution or on a grid 2^L times coarser with averaged colours; vc_fetch_shell_viewer turns the list into the
 * float32 arrays the reference's viewer draws (assignment.py:127-133), on the device.  The result is left exactly as it is.  The
 * contract, bit for bit (tests/shell_np.py restates it).
 *   Grid: nx, ny, nz cells, linear index i = (iz nx + ix) ny + iy.  ON = a survivor of the current carve result as
 *   vc_fetch_occupancy sees it (photo carve, components, morphology, grow, temporal vote and footprint rules included).
 *   1 level: L in 0 .. VC_SHELL_MAX_LEVEL, f = 2^L.  The coarse grid has n'_a = ceil(n_a / f) cells per axis; coarse cell
 *     (cx, cy, cz) covers the fine indices f c <= i_a < min(f c + f, n_a) per axis, is ON when any of its voxels is ON, and has
 *     the index j = (cz nx' + cx) ny' + cy.  At L = 0 the coarse grid is the grid.
 *   2 faces: one byte per ON cell; bits 0 .. 5 stand for -x, +x, -y, +y, -z, +z (the order of vc_measure_t::faces); a bit is set
 *     when the neighbour across that face is OFF or outside the (coarse) grid.  Nothing wraps around.  The shell is the set of ON
 *     cells with a non-zero face byte.
 *   3 shell records: the shell cells in ascending j, 8 bytes each, {u32 j, u8 r, g, b, seen}.  At L = 0 bytes 4 .. 7 are the
 *     survivor's record bytes unchanged.  At L > 0, with n = the level-0 shell voxels inside the cell whose seen byte has bit 0
 *     set: n > 0 gives each channel as (sum c + n / 2) / n in unsigned integers (floor) and seen = 1; n = 0 gives 0, 0, 0, 0.
 *     (Every coarse shell cell holds a level-0 shell voxel, so n = 0 only where the colour camera sees none of them.)
 *   4 viewer arrays: `scaling` a double, the axes A = xs, ys, zs of vc_get_axes.  Per axis lo = f c, hi = min(f c + f, n_a) - 1,
 *     v_a = (trunc(A[lo]) / scaling + trunc(A[hi]) / scaling) * 0.5 in float64; position = {(float)v_x, (float)(-v_z),
 *     (float)v_y}, colour_k = (float)((double)c_k / 255.0).  At L = 0 these are the reference's arrays of the same voxels bit for
 *     bit ((a + a) * 0.5 = a).  At L > 0 the caller draws cubes f times as large: stats.cube_scale = f.
 *   5 a read-only pass: records, count and occupancy stay; the result generation does not advance, so the products of the other
 *     passes stay valid.  vc_fetch_shell and vc_fetch_shell_viewer fail ("no shell") until the pass has run on the current result
 *     and again after anything that changes which voxels survive.  Colour passes (vc_color_visible, vc_paint_clusters,
 *     vc_paint_geodesic) leave the shell valid: it holds the colours the records had at the call, so run it after the colouring.
 *     VC_ERR_ARG (with a message, nothing launched) when there is no carve result, steps are in flight, the carve ran with
 *     VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of more than one rank is attached, L >
 *     VC_SHELL_MAX_LEVEL, flags != 0, stats == NULL, or the grid exceeds the u32 index.  S = 0 is no error.  Synchronous, with
 *     one read-back (the count) before the shell's buffers are sized; VC_ERR_OOM when they cannot be, the result as it was.
 * stats (required): survivors = S; cells_on = the ON cells of the (coarse) grid (S at L = 0); shell = T, the cells listed;
 * faces[k] = the shell cells with bit k set; level, cube_scale = 2^level, dims = the (coarse) grid; shell_ms = HIP events around
 * the whole call.  vc_fetch_shell: either pointer may be NULL (both: only asks whether the shell is valid).
 * vc_fetch_shell_viewer builds both arrays on the device and copies 24 bytes per shell record; either pointer may be NULL;
 * VC_ERR_ARG when scaling is 0 or not finite. */
#define VC_SHELL_MAX_LEVEL 6u
typedef struct {
    uint64_t survivors, cells_on, shell;
    uint64_t faces[6];
    uint32_t level, cube_scale, dims[3];
    float shell_ms;                 /* HIP events around the whole call */
} vc_shell_stats_t;
int vc_hull_shell(vc_ctx *ctx, uint32_t level, uint32_t flags /* must be 0 */, vc_shell_stats_t *stats);
int vc_fetch_shell(vc_ctx *ctx, uint64_t *records /* [shell] */, uint8_t *faces /* [shell] */);
int vc_fetch_shell_viewer(vc_ctx *ctx, double scaling, float *positions /* [shell][3] */, float *colors /* [shell][3] */);

/* ---- the hull thinned to a curve skeleton, topology kept (no reference counterpart) ---------------------------------------------------
 * vc_hull_thin peels the current carve result, as vc_fetch_occupancy and vc_fetch_records see it, down to a centred, one-voxel-wide
 * skeleton with the components, tunnels and cavities of the hull.  The result is left exactly as it is: the pass works on a copy
 * of the occupancy.  The contract, bit for bit (tests/thin_np.py restates it).  Integers and bits only.
 *   1 the object is the set H of survivors; everything outside the grid is background; connectivity is 26 for H and 6 for the
 *     background.  N26*(p) = the 26 neighbours of p, N18*(p) = those that differ from p in at most two coordinates, the
 *     6-neighbours = those that differ in one.
 *   2 p is simple when H n N26*(p) has exactly one 26-connected component (adjacency inside N26*(p)) and (complement of H) n
 *     N18*(p) has exactly one 6-connected component (adjacency inside N18*(p)) that contains a 6-neighbour of p.  A voxel with no
 *     neighbour in H is not simple.  p is an end point when it has exactly one neighbour in H.
 *   3 directions, as offsets in (ix, iy, iz): d0 .. d5 = (0,0,-1), (0,0,+1), (0,-1,0), (0,+1,0), (-1,0,0), (+1,0,0).  The
 *     subfield of a voxel is s = (ix & 1) | (iy & 1) << 1 | (iz & 1) << 2.
 *   4 a pass is six direction steps d0 .. d5.  At its start a direction step marks as candidates the voxels of H that are no
 *     anchors and whose neighbour p + d is background; then eight sub-steps s = 0 .. 7 follow, and sub-step s removes from H, all
 *     at once, every candidate of subfield s that is simple in the H of that moment -- and, with mode VC_THIN_CURVE, no end point
 *     in that H.  VC_THIN_POINT has no end-point condition: a component shrinks to a topological kernel (a ball to a point, a
 *     torus to a ring, a shell to a closed surface).  Passes repeat until one removes nothing or max_passes of them have run
 *     (1 <= max_passes <= VC_THIN_MAX_PASSES; the last pass of a stable result is the one that removed nothing).  Two voxels of a
 *     subfield are never 26-neighbours and the predicate reads N26* alone, so a sub-step equals the removal of its voxels one by
 *     one in any order: every removal is of a simple voxel, and no order of evaluation shows.
 *   5 anchors are never removed.  anchor_source VC_THIN_ANCHORS_NONE: none (`anchors`, `n_anchors` ignored).
 *     VC_THIN_ANCHORS_LIST: n_anchors linear indices, duplicates allowed, every one a survivor.  VC_THIN_ANCHORS_EXTREMA: the
 *     voxels at distance 0 of a vc_hull_geodesic that is current: its seed set and its extremities.
 *   6 outputs.  Per record peel (u16): 0 for a kept voxel, else 1 + 6 (pass - 1) + d of the direction step that removed it (pass
 *     from 1).  Per kept voxel, ascending by voxel index, a vc_skeleton_voxel_t {voxel, record, degree = the kept voxels in
 *     N26*}.  Bit c of the table of vc_fetch_thin_table (byte c >> 3, bit c & 7) says whether a voxel whose neighbourhood has the
 *     code c is simple; bit k of a code is the neighbour at offset (dx, dy, dz) with k27 = (dz + 1) 9 + (dx + 1) 3 + (dy + 1),
 *     k = k27 below 13 and k27 - 1 above it.
 *   7 VC_ERR_ARG (with a message; the outputs of an earlier call are gone once the arguments have passed) when there is no carve
 *     result, steps are in flight, the carve ran with VC_FLAG_NO_RECORDS, the slab is narrower than the grid, a communicator of
 *     more than one rank is attached, mode, anchor_source or flags (must be 0) is unknown, stats == NULL, max_passes is out of
 *     range, the grid exceeds the u32 index, anchors == NULL with n_anchors > 0, an anchor is no survivor (the message names the
 *     first such position and its voxel), or VC_THIN_ANCHORS_EXTREMA comes without a current vc_hull_geodesic.  S = 0 is no
 *     error.  Synchronous.
 *   8 lifetime: vc_fetch_thin and vc_fetch_skeleton fail ("no skeleton") until the pass has run on the current result and again
 *     after anything that changes which voxels survive, as vc_fetch_component_labels does; colour passes leave them valid, and
 *     so does a later vc_hull_geodesic: a skeleton anchored at VC_THIN_ANCHORS_EXTREMA keeps the anchors of the geodesic pass that
 *     was current at the call.
 * Two routes evaluate the predicate, with equal bytes: in registers (option thin_table = 0, the default until the table has been
 * measured faster) or by a look-up in the table of 2^26 bits, which a kernel builds with the same function at first use
 * (thin_table = 1).  stats (required): survivors; anchors = the distinct anchor voxels; kept, removed; passes = passes run;
 * steps = direction steps that had a candidate; launches = kernels the call launched (it depends on the route taken and is no
 * part of the restated contract); stable = 0 when max_passes cut the thinning short; isolated / endpoints / junctions = kept
 * voxels of degree 0 / 1 / >= 3; thin_ms = HIP events around the whole call. */
#define VC_THIN_CURVE 0u
#define VC_THIN_POINT 1u
#define VC_THIN_ANCHORS_NONE    0u
#define VC_THIN_ANCHORS_LIST    1u
#define VC_THIN_ANCHORS_EXTREMA 2u
#define VC_THIN_MAX_PASSES 10000u
#define VC_THIN_DEFAULT_PASSES 4096u
#define VC_THIN_TABLE_BYTES (1u << 23)
typedef struct {
    uint32_t voxel, record;
    uint8_t degree, pad[3];         /* pad: zeros */
} vc_skeleton_voxel_t;
typedef struct {
    uint64_t survivors, anchors, kept, removed;
    uint64_t isolated, endpoints, junctions;
    uint32_t passes, steps, launches, stable;
    float thin_ms;                  /* HIP events around the whole call */
} vc_thin_stats_t;
int vc_hull_thin(vc_ctx *ctx, uint32_t mode, uint32_t anchor_source, const uint32_t *anchors /* [n_anchors], VC_THIN_ANCHORS_LIST only */,
                 uint64_t n_anchors, uint32_t max_passes, uint32_t flags /* 0 */, vc_thin_stats_t *stats);
int vc_fetch_thin(vc_ctx *ctx, uint16_t *peel);                            /* [S] */
int vc_fetch_skeleton(vc_ctx *ctx, vc_skeleton_voxel_t *out);              /* [stats.kept] */
int vc_fetch_thin_table(vc_ctx *ctx, uint8_t *bits);                       /* [VC_THIN_TABLE_BYTES]; builds the table if need be */

/* ---- the step before the path ---------------------------------------------------------------------------------
 * extract_foreground_mask, background_subtraction.py:129-208, on the device: the front half (:153-168) by the calls below, the
 * contour stage (:171-193) by vc_fill_figures, the 2x2 post-filter and the final threshold (:195-206) by the carve path's own
 * preparation (vc_set_mask_postfilter); vc_foreground_to_slot chains all of it into a carve slot.  Host buffers in and out
 * except for vc_foreground_to_slot.
 * vc_bgr_to_hsv: replaces cv2.cvtColor(image, cv2.COLOR_BGR2HSV) (:155) on uint8 [H,W,3] -- OpenCV's 8-bit fixed-point
 * conversion (H in 0..179).  vc_mask_morphology: replaces cv2.morphologyEx(mask, MORPH_OPEN / MORPH_CLOSE,
 * getStructuringElement(MORPH_RECT, (ksize, ksize))) on uint8 [H,W], opening first when both flags are set: ksize 3 = the
 * pre-filter (:161-168), ksize 2 = the post-filter (:195-203; the carve path applies that one itself on upload, see
 * vc_set_mask_postfilter).  Parity with cv2 is unpinned (oracle/foreground_np.py restates OpenCV's published code). */
int vc_bgr_to_hsv(vc_ctx *ctx, const uint8_t *bgr, uint32_t H, uint32_t W, uint8_t *hsv);
int vc_mask_morphology(vc_ctx *ctx, const uint8_t *mask, uint32_t H, uint32_t W, uint32_t ksize, int open, int close, uint8_t *out);
/* The background model between them: cv2.bgsegm.createBackgroundSubtractorMOG(history, nmixtures, backgroundRatio, noiseSigma)
 * (background_subtraction.py:75-76; assignment.py:79 trains one per camera) and its apply(image, None, learningRate)
 * (:91 training, :158 inference with learning rate 0) on uint8 [H,W,3] images -> uint8 [H,W] {0, 255}.  The model lives on the
 * device (8 floats per mixture and pixel); it starts over on its first frame, on a learning rate >= 1 and when the image size
 * changes; a negative learning rate means 1 / min(frames seen, history), as in OpenCV.  Non-positive constructor arguments select
 * OpenCV's defaults (history 200, 5 mixtures (at most 8), backgroundRatio 0.95 when not given, noiseSigma 15).  vc_mog_state
 * copies the model out ([8 nmixtures][H W] float planes: plane 8 k + f = field f of component k; f: 0 sort key, 1 weight,
 * 2..4 mean, 5..7 variance; state may be null to ask for the sizes only) -- tests and persistence.  Restated from the published
 * algorithm of opencv_contrib's bgsegm module (bgfg_gaussmix.cpp); parity with cv2 unpinned (oracle/mog_np.py). */
#define VC_MAX_MOG_MODELS 64
int vc_mog_create(vc_ctx *ctx, int history, int nmixtures, double background_ratio, double noise_sigma, uint32_t *model);
int vc_mog_apply(vc_ctx *ctx, uint32_t model, const uint8_t *image, uint32_t H, uint32_t W, double learning_rate, uint8_t *fgmask);
int vc_mog_state(vc_ctx *ctx, uint32_t model, float *state, uint64_t capacity, uint32_t *H, uint32_t *W, uint32_t *nmixtures, uint32_t *nframes);
int vc_mog_destroy(vc_ctx *ctx, uint32_t model);
/* The MOG2 model: cv2.createBackgroundSubtractorMOG2(history, varThreshold, detectShadows) (background_subtraction.py:90-127, the
 * comparison script :398-401 with history = frame count, varThreshold 650, detectShadows false) and its apply(image, None,
 * learningRate) on uint8 [H,W,3] -> uint8 [H,W] {0, shadow_value, 255}.  Non-positive history / var_threshold select OpenCV's
 * 500 / 16; the other arguments are the model's fixed defaults in OpenCV (5 mixtures, backgroundRatio 0.9, varThresholdGen 9,
 * varInit 15, varMin 4, varMax 75, complexityReductionThreshold 0.05, shadowValue 127, shadowThreshold 0.5), stored as OpenCV
 * stores them (float; varThreshold as double((float)v)).  nmixtures must lie in 1..8 (a limit of this build, VC_ERR_ARG beyond)
 * and shadow_value in 0..255.  The model starts over on its first frame, on a learning rate >= 1 and when the image size changes;
 * a negative learning rate means 1 / min(2 frames seen, history).  Unlike MOG, learning rate 0 still writes the model (weights
 * renormalised).  Handles are VC_MOG2_MODEL_TAG | index (at most VC_MAX_MOG_MODELS of them); vc_foreground_front and
 * vc_foreground_to_slot take either kind, the vc_mog_* calls only MOG handles and the vc_mog2_* calls only MOG2 handles.
 * vc_mog2_state copies the model out: state [5 nmixtures][H W] float planes (plane 5 k + f = field f of component k; f: 0
 * weight, 1 variance, 2..4 mean), nmodes [H W] u8 (components in use per pixel; those beyond keep their last values); either
 * buffer may be null, both null asks for the sizes only.  Restated from the published CPU path of OpenCV's bgfg_gaussmix2.cpp;
 * parity with cv2 unpinned (tests/mog2_np.py). */
#define VC_MOG2_MODEL_TAG 0x10000u
int vc_mog2_create(vc_ctx *ctx, int history, double var_threshold, int detect_shadows, int nmixtures, double background_ratio,
                   double var_threshold_gen, double var_init, double var_min, double var_max, double complexity_reduction_threshold,
                   int shadow_value, double shadow_threshold, uint32_t *model);
int vc_mog2_apply(vc_ctx *ctx, uint32_t model, const uint8_t *image, uint32_t H, uint32_t W, double learning_rate, uint8_t *fgmask);
int vc_mog2_state(vc_ctx *ctx, uint32_t model, float *state, uint64_t capacity, uint8_t *nmodes, uint64_t nmodes_capacity, uint32_t *H,
                  uint32_t *W, uint32_t *nmixtures, uint32_t *nframes);
int vc_mog2_destroy(vc_ctx *ctx, uint32_t model);
/* Everything of extract_foreground_mask in front of the contour stage in one call, one copy each way: BGR -> HSV where to_hsv
 * (:155; the reference always does), the model's apply with `learning_rate` (:158), the 3x3 opening / closing where asked
 * (:161-168).  bgr uint8 [H,W,3] in, the model's mask uint8 [H,W] out (a MOG2 model's shadows stay shadow_value: the
 * 3x3 filter keeps grey levels, and every later stage takes != 0 as foreground, as cv2.findContours does). */
int vc_foreground_front(vc_ctx *ctx, uint32_t model, const uint8_t *bgr, uint32_t H, uint32_t W, int to_hsv, double learning_rate,
                        int open, int close, uint8_t *mask);
/* The contour stage, background_subtraction.py:171-193: cv2.findContours(mask, RETR_TREE, CHAIN_APPROX_SIMPLE), every contour
 * with contourArea >= figure_threshold drawn and filled with 255, each of its children with contourArea(child, True) >=
 * inner_threshold filled with 0 and its outline drawn again.  mask uint8 [H,W] (foreground where != 0) in, uint8 [H,W] {0, 255}
 * out.  Computed from connected components, the component tree and per-cell areas instead of border following (csrc/vc_contour.h);
 * held to a literal restatement of Suzuki-Abe border following, fillPoly and drawContours (tests/contour_literal.py), parity with
 * cv2 itself unpinned. */
int vc_fill_figures(vc_ctx *ctx, const uint8_t *mask, uint32_t H, uint32_t W, double figure_threshold, double inner_threshold,
                    uint8_t *out);
/* extract_foreground_mask of every camera into a carve slot without a host round trip, background_subtraction.py:129-208 as
 * assignment.py:98-109 calls it: camera c's BGR image bgr[c] ([C][H][W][3], the vc_set_cameras size) goes through BGR -> HSV, the
 * apply of background model models[c] with learning_rate (:155-158), the 3x3 opening / closing where open_pre[c] / close_pre[c]
 * (:161-168; NULL = none) and the contour stage with figure_thr[c], inner_thr[c] (:171-193); the masks land in the slot's byte
 * masks and the images in its frames (any camera can colour the records).  The 2x2 post-filter and the final threshold
 * (:195-206) are the slot's preparation in front of the next carve (vc_set_mask_postfilter), as after vc_upload_masks.
 * n_models >= C.  ASYNCHRONOUS like vc_upload_masks: one staged copy of the C images, then kernels on the upload stream. */
int vc_foreground_to_slot(vc_ctx *ctx, uint32_t slot, const uint32_t *models, uint32_t n_models, const uint8_t *bgr, uint32_t H,
                          uint32_t W, double learning_rate, const double *figure_thr, const double *inner_thr, const uint8_t *open_pre,
                          const uint8_t *close_pre);

/* ---- the step after the path: marching cubes over the dense ON/OFF volume -------------------------------
 * Replaces skimage.measure.marching_cubes(voxels_status, 0) of plot_marching_cubes, voxel_reconstruction.py:127-163, whose
 * input the reference builds as the statuses in voxel order reshaped to (width, height*2, depth) (assignment.py:143-146).
 * volume_bits: d0*d1*d2 bits, element i = bit (i & 7) of byte i >> 3, C order (axis 2 fastest); NULL = the occupancy of
 * the last carve of this context, viewed as a (d0, d1, d2) array over the voxel index (d0*d1*d2 must equal the slab's
 * voxel count: (nx, ny, nz) is literally the reference's reshape, (nz, nx, ny) the geometric axes).  Vertices lie on the
 * cube edges between an ON and an OFF element at off + level * (on - off), 0 <= level < 1 (the reference passes 0), in
 * index coordinates (axis 0, 1, 2); faces index them, oriented from ON to OFF.  Classic table-driven marching cubes; the
 * table is generated (csrc/mc_table.h), NOT scikit-image's Lewiner variant: parity with skimage is unpinned. */
int vc_marching_cubes(vc_ctx *ctx, const uint8_t *volume_bits, uint32_t d0, uint32_t d1, uint32_t d2, float level,
                      uint64_t *n_verts, uint64_t *n_faces);
/* verts: float [n_verts][3], faces: u32 [n_faces][3] of the last vc_marching_cubes; either may be NULL. */
int vc_fetch_mesh(vc_ctx *ctx, float *verts, uint32_t *faces);

/* ---- silhouette-refined, coloured surface mesh of the current result (no reference counterpart) ---------------------------------
 * vc_surface_mesh meshes the current carve result as vc_fetch_occupancy sees it (vc_color_visible, vc_photo_carve and
 * vc_hull_components included) in world millimetres, each vertex moved along its grid edge to where the silhouettes cross it.
 * The contract, bit for bit (tests/surface_np.py restates it); float64 with no contraction, in the order written:
 *   1 topology: the vertices and faces of vc_marching_cubes(NULL, nz, nx, ny) on the same result, same order; vertex axes
 *     (iz, ix, iy) -> (z, x, y), a cyclic permutation, so faces stay oriented from ON to OFF (outward, positive signed volume).
 *   2 point test: T(P) = the cameras c with off = pixel_offset(project_point(cam_c, P), H, W) >= 0 and mask_bit(bits_c, off),
 *     bits_c = camera c's mask of the carve's frame set after its 2x2 post-filter (what the carve read); P is inside iff
 *     T(P) >= m, m = the carve's min_views after its clamp to >= 1.
 *   3 edge points: a vertex's edge joins an ON and an OFF element; P_on and P_off are their voxel centres on the carve's
 *     linspace axes, differing in one coordinate a.  P(s)_a = on_a + s * (off_a - on_a) (two roundings), the other two
 *     coordinates the shared ones; P(0) = P_on and P(1) = P_off by definition (the centres the carve tested).
 *   4 bisection: a vertex is refined iff T(P_on) >= m and T(P_off) < m.  Then lo = 0, hi = 1 and for k = 1 .. steps:
 *     mid = (lo + hi) * 0.5, lo = mid if P(mid) is inside else hi = mid; s = (lo + hi) * 0.5.  Otherwise (a photo carve or a
 *     foreign lookup table made the occupancy disagree with the point test) s = 0.5.  steps = 0 gives s = 0.5 everywhere.
 *     Every s is dyadic: the arithmetic on it is exact.
 *   5 outputs, fetched by vc_fetch_surface_mesh (any pointer may be NULL): verts f64 [V][3] = P(s) as world (x, y, z) mm;
 *     faces u32 [F][3]; rgb u8 [V][3] = the RGB of the ON element's record; refined u8 [V] (0 / 1).
 * stats (required): n_verts, n_faces, refined, unrefined (contract); point_tests = camera tests the device evaluated (a
 * diagnostic: it stops a vertex's test once T >= m or T < m is decided; option surface_order); surface_ms = HIP events
 * around the whole call.  VC_ERR_ARG (with a message) when there is no carve result, steps are in flight, the carve ran with
 * VC_FLAG_NO_RECORDS, a communicator of more than one rank is attached, the slab is narrower than the grid, steps > 24,
 * flags != 0, stats == NULL, or the carve's frame set has been prepared again since the carve (its masks are no longer the
 * ones the occupancy came from).  An empty hull is no error (V = F = 0).  Synchronous, one read-back (the counts) in the middle.
 * The mesh stays valid until the next vc_surface_mesh (a refused one included) or vc_destroy; a new carve does not touch it, and
 * vc_fetch_mesh still returns the last vc_marching_cubes mesh.  vc_fetch_surface_mesh fails when there is no mesh. */
typedef struct {
    uint64_t n_verts, n_faces;      /* contract */
    uint64_t refined, unrefined;    /* contract: refined + unrefined = n_verts */
    uint64_t point_tests;           /* diagnostic, implementation-defined */
    float surface_ms;               /* HIP events around the whole call */
} vc_surface_stats_t;
int vc_surface_mesh(vc_ctx *ctx, uint32_t steps, uint32_t flags, vc_surface_stats_t *stats);
int vc_fetch_surface_mesh(vc_ctx *ctx, double *verts, uint32_t *faces, uint8_t *rgb, uint8_t *refined);

/* Tuning knobs: which of the equivalent kernels runs and with what launch geometry; NEVER changes results
 * (tests/test_gpu_parity.py::test_every_kernel_family_agrees_with_oracle runs every kernel family against the oracle at 4
 * cameras; tests/test_gpu_camera_counts.py runs the same list at 6, 7, 9, 11, 13 and 15 cameras, voxel_pairs and dbg 8192 /
 * 16384 at 1 to 16 cameras, grid_lds_kb on both sides of every LDS edge of the brick pipeline at 4, 5, 9 and 16 cameras, and
 * the launch-shape knobs, voxel_batches and overlap at their limits on a grid whose minimum launches stride).  Defaults are
 * the measured best on MI355X.
 *   kernel choice   lut_hier (1)  hierarchical lookup-table kernel, 0 = stream the table (k_lut_first + refine)
 *                   lut_tile, fused_tile (1)  words of 4 x-rows x 16 y where nx % 4 == 0 and ny % 64 == 0
 *                   bricks (1)  ny in {256, 512, 1024, 2048, 4096}: the brick pipeline (whole 16^3-voxel bricks decided from their pixel
 *                                  boxes, flat lists of bricks / undecided words / columns, one launch per level) instead of
 *                                  the one-launch hierarchical kernels
 *                   cull (1)  the one-launch kernels on tile words skip whole bricks too (k_cull); 0 also switches `bricks` off
 *                   fused_hier (1), fused_boxes (1), fused_f32box (1)  table-free kernel: word rejection; boxes read /
 *                                  bounded on the fly in float32 / float64 intervals
 *                   fused_color_table (1)  table-free carve, survivors coloured from the colour camera's table (4 B per
 *                                  voxel of the whole grid, ONE camera, projected at the first step that wants it) instead of
 *                                  by projecting each of them again; 0: no table of any kind (the expansion is then FP64-bound)
 *                   refine_pair (1), reorder (1)  two cameras per round trip; most selective camera first
 *                   voxel_pairs (0)  per-voxel level of the brick pipeline: 0 = two cameras per round trip up to 4 cameras, one
 *                                  above; 1 = always two; 2 = always one
 *                   voxel_batches (0 = 8 for table look-ups with two cameras per round, else 1)  batches of 8 undecided words a wave of
 *                                  the per-voxel level takes one after the other
 *                   emit_lanes (1), emit_busy (1: grids >= 64 M voxels, 2: always, 0: never)  record expansion form
 *                   force_generic (0)  one thread per voxel everywhere (also env VOXCARVE_FORCE_GENERIC=1)
 *                   emit_lut16 (1)  VC_MODE_LUT on a tile-ordered table (ny in {64, 128, 256, 512, 1024}): the expansion reads the
 *                                  colour camera's entries as 16-bit differences to the smallest offset of their tile word, from a
 *                                  compact copy (2 B per voxel of the slab + 4 B per 64) packed by the first step that names the
 *                                  camera; a camera whose tile words span more than 65534 pixels of offset, or a device without
 *                                  the memory, keeps the 4-byte entries.  0: 4-byte entries always.  Same records either way;
 *                                  read by the next vc_carve_begin (vc_debug_counters out[6] tells which a step took)
 *   frame sets      grid_lds_kb (0 = 16; frame sets above 2 MB of mask bits: what their uncropped grids need at the finest block
 *                                  that fits 148 KB, brick pipeline, or 64 KB, other kernels; explicit values above 64 are
 *                                  clamped to 64 for those), grid_min_shift (1)  LDS budget / finest block of the cropped
 *                                  block grids (read when a frame set is next prepared)
 *   launch shape    hier_blocks_per_cu (48), emit_waves_per_cu (256), first_kv (1), first_blocks_per_cu (3),
 *                   refine_b (8), refine_blocks_per_cu (8), fused_blocks_per_cu (8)
 *   streams         overlap (1)  scan + record expansion of a step on a second stream, beside the next step's carve
 *                                  (single stream while a communicator is attached)
 *   colouring       visible_check (1)  vc_color_visible's splats read the stored depth and skip the atomic when it is already at or
 *                                  below theirs; visible_big_rect (64)  splat rectangles of more pixels get a workgroup each
 *   rendering       render_blocks (1)  vc_render skips empty blocks of 8^3 voxels whole; 0: one cell per step everywhere
 *   meshing         surface_order (1)  vc_surface_mesh's bisection tries the cameras that rejected P_off first; 0: camera order
 *   clusters        cluster_floor_records (1)  vc_hull_clusters builds its floor map by one atomic per record, the faster way
 *                                  as measured; 0: from the occupancy words (the same map; scripts/exp_clusters.py times both)
 *   geodesic        geodesic_tiles (1)  vc_hull_geodesic relaxes by tiles held in LDS, one workgroup per listed tile and launch;
 *                                  0: by sweeps of one lane per record over the whole hull (the same bytes;
 *                                  scripts/exp_geodesic.py times both)
 *   thinning        thin_table (0)  vc_hull_thin evaluates the simple-point predicate in registers; 1: looks it up in the table
 *                                  of 2^26 bits built on the device at first use (the same bytes; scripts/exp_thin.py times both)
 *   experiments     dbg (0)  bit 0: skip the per-voxel level (undecided words count as alive), bit 1: skip the word level
 *                                  too -- WRONG results on purpose, to time the levels apart (scripts/exp_bricks.py); bit 2:
 *                                  no word-level tests, every word of a listed brick goes to the per-voxel level (right results)
 *                                  bit 13: the brick level lists every brick without testing (what it does by itself once a step has
 *                                  listed nine bricks in ten), bit 14: wide frame sets without the survivors' compaction at the word
 *                                  level -- right results, other paths (tests)
 *   timing          timing_detail (0)  1: vc_carve_begin steps record the events around preparation and carve kernels too
 *                                  (vc_carve always does; see vc_timing_t), every kernel carries begin / end events on its own
 *                                  launch (kernel_ms_sum) and counts its work (vc_timing_t::work)
 *                   kernel_events (0)  1: only the per-launch begin / end events (kernel_ms_sum, kernel_launches) of the kernels of
 *                                  carve steps, nothing else changes; the launches of the post-carve passes (VC_K_DIST_BOX and
 *                                  above) carry theirs under timing_detail alone
 *   streams         stream_priority (1)  carve + preparation streams at the highest queue priority, the expansion stream at
 *                                  the lowest (the expansion fills every wave slot; the carve chain is a row of short launches
 *                                  that would queue behind it); launch_events (1)  the events the streams exchange ride on
 *                                  the launches in front of them; event_scope (1)  those events release to the device only;
 *                                  reserve_cus (0)  k compute units per XCD kept out of the expansion stream's CU mask
 *   multi-GPU       gather_compact (1)  exchange occupancy words instead of records;
 *                   gather_sync (1)  0: vc_allgather returns once its work is queued (two gathers may be in flight; a read-back,
 *                                  vc_timing or vc_synchronize waits for them; vc_fetch_gathered returns the last one's list)
 * Unknown names or out-of-range values return VC_ERR_ARG. */
int vc_set_option(vc_ctx *ctx, const char *name, int value);
int vc_timing(vc_ctx *ctx, vc_timing_t *out);
/* sizeof(vc_timing_t) as the library was built: a binding checks its own mirror of the struct against it before the first call. */
uint32_t vc_timing_struct_size(void);
/* Diagnostics of the last brick-pipeline carve (scripts/, DESIGN figures): out[0] bricks listed for a look at their words,
 * out[1] bricks that may hold survivors, out[2] bricks whose voxels all survive, out[3] bricks of the slab, out[4] brick
 * columns listed, out[5] tile words that took the per-voxel test; out[6] 1 when the record expansion launched last read the colour
 * camera's compact table (option emit_lut16), out[7] 1 while such a table exists. */
int vc_debug_counters(vc_ctx *ctx, uint64_t out[8]);
int vc_timing_reset(vc_ctx *ctx);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI (no reference counterpart) ---- */
int vc_comm_unique_id(uint8_t out[VC_UNIQUE_ID_BYTES]);
int vc_comm_init(vc_ctx *ctx, int n_ranks, int rank, const uint8_t uid[VC_UNIQUE_ID_BYTES]);
int vc_comm_destroy(vc_ctx *ctx);
/* All-gather of every rank's survivor records in rank (= z-slab = index) order.
 * counts_out (NULL ok): n_ranks entries.  *total_out = global survivor count.
 * What crosses xGMI is the compact form below (option "gather_compact", default 1): each rank's
 * non-zero occupancy words; every rank expands all of them into the full record list itself, taking
 * colours from its own copy of the colour camera's table over the whole grid (VC_MODE_LUT: 4 B per
 * voxel of the whole grid, built at the first call) or by re-projection (VC_MODE_FUSED).  With the
 * option off the 8-byte records themselves are exchanged. */
int vc_allgather(vc_ctx *ctx, uint64_t *counts_out, uint64_t *total_out);
/* The compact form for host-side transports (and tests): entries = pairs of u64 {occupancy bits of one
 * 64-voxel word, global linear index of its bit 0}, non-zero words only, ascending.
 * vc_pack_entries packs the last carve's slab; vc_fetch_entries copies 2*n u64 out;
 * vc_expand_entries takes the concatenation of all ranks' entries in rank order and leaves the ordered
 * records of the whole grid where vc_fetch_gathered reads them, coloured like the last carve of THIS
 * context (same mode, colour camera and frame set). */
int vc_pack_entries(vc_ctx *ctx, uint64_t *n_entries_out);
int vc_fetch_entries(vc_ctx *ctx, uint64_t *entries);
int vc_expand_entries(vc_ctx *ctx, const uint64_t *entries, uint64_t n_entries, uint64_t *total_out);
int vc_fetch_gathered(vc_ctx *ctx, uint64_t *records);
/* Max of one double over all ranks via RCCL (doubles as a barrier for host code). */
int vc_comm_allreduce_max(vc_ctx *ctx, double *inout);

#ifdef __cplusplus
}
#endif
#endif /* VOXCARVE_H */
