// libvoxcarve.so -- MI355X (gfx950) visual-hull carve engine: kernels + C ABI.
//
// Path replaced (reference root = ChristosP1/Voxel-Based-3D-Reconstruction):
//   create_voxel_volume                        voxel_reconstruction.py:35-59
//   create_lookup_table (cv2.projectPoints)    voxel_reconstruction.py:62-86
//   update_visible_voxels_and_extract_colors   voxel_reconstruction.py:89-124
//   selection loop of set_voxel_positions      assignment.py:116-133
//
// Data layout in HBM (per context = per rank = one z-slab of n voxels, slab-local j):
//   axes      f64 xs[nx], ys[ny], zs[nz]        np.linspace tables (host-built, exact)
//   maskbits  u32 [slot][C][ceil(H*W/32)]       bit b of word w = pixel 32w+b foreground
//   frames    u8  [slot][C][H*W*3]              BGR, only the colour camera is read
//   lut       i32 [C][n]                        pixel offset or -1 (VC_MODE_LUT)
//   words     u64 [ceil(n/64)]                  survivor bit per voxel (= dense occupancy)
//   groupcnt  u32 [n_pad/4096]                  survivors per group of 64 words
//   groupoff  u32 [groups], blockoff u64        two-level exclusive scan of groupcnt
//   records   u64 [S]                           {u32 idx, r, g, b, seen}, ascending idx
//
// There is no CPU path in this library: without a GPU vc_create fails (VC_ERR_NODEV).
//
// Layout: the kernels' headers, then the host side in dependency order.  The core (vc_ctx, the launch helpers, set-up, the carve step,
// the pass frame) and the passes up to the set algebra stand in this file; every later family lives in a file of its own under host/,
// included once where its code stood; behind them the foreground front end, the options and the multi-GPU calls, in this file again.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only; the functions are resolved with dlsym

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/voxcarve.h"
#include "vc_kernels.h"
#include "vc_mc.h"
#include "vc_fg.h"
#include "vc_contour.h"
#include "vc_visible.h"
#include "vc_compact.h"
#include "vc_photo.h"
#include "vc_components.h"
#include "vc_render.h"
#include "vc_surface.h"
#include "vc_footprint.h"
#include "vc_distance.h"
#include "vc_grow.h"
#include "vc_temporal.h"
#include "vc_setops.h"
#include "vc_motion.h"
#include "vc_motion_pyramid.h"
#include "vc_temporal_motion.h"
#include "vc_normals.h"
#include "vc_texture.h"
#include "vc_light.h"
#include "vc_clusters.h"
#include "vc_geodesic.h"
#include "vc_measure.h"
#include "vc_thin.h"
#include "vc_shell.h"
#include "vc_owned.h"

#pragma clang fp contract(off)

using namespace vc;

namespace {

// ================================================================ host side
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi g_rccl;
std::string g_create_error;

// RCCL is resolved at first use so single-GPU runs never load it, and so that a
// process which already holds a librccl.so.1 (any host framework) shares that copy.
bool load_rccl(std::string &err)
{
    if (g_rccl.handle) return true;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { err = std::string("dlopen librccl: ") + dlerror(); return false; }
#define VC_SYM(field, name)                                                             \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name));            \
    if (!g_rccl.field) { err = std::string("dlsym ") + name + " failed"; return false; }
    VC_SYM(GetUniqueId, "ncclGetUniqueId")
    VC_SYM(CommInitRank, "ncclCommInitRank")
    VC_SYM(CommDestroy, "ncclCommDestroy")
    VC_SYM(AllGather, "ncclAllGather")
    VC_SYM(Broadcast, "ncclBroadcast")
    VC_SYM(AllReduce, "ncclAllReduce")
    VC_SYM(GroupStart, "ncclGroupStart")
    VC_SYM(GroupEnd, "ncclGroupEnd")
    VC_SYM(GetErrorString, "ncclGetErrorString")
#undef VC_SYM
    g_rccl.handle = h;
    return true;
}

// Scratch of one scan_counts: counts and exclusive offsets per group, sums and offsets of the scan blocks
struct ScanBufs {
    DevBuf<uint32_t> cnt, off;
    DevBuf<uint64_t> bsum, boff;
};

// One resident frame set.  The uploaded bytes stay on the device (bytes / fbytes), so the derived state (bit masks,
// record-layout images, block grids, camera order -- all made on the device by k_prep_pack / k_prep_grid, queued in front of
// the first carve that uses the slot) can be re-derived without another transfer (vc_touch_masks).
struct Slot {
    DevBuf<uint8_t> bytes;      // [C][H*W] byte masks as uploaded
    Pinned<uint8_t> h_bytes;    // page-locked staging of the same size: uploads are asynchronous
    DevBuf<uint8_t> fbytes[VC_MAX_CAMERAS];   // [H*W*3] BGR image of a camera as uploaded
    Pinned<uint8_t> h_fbytes[VC_MAX_CAMERAS];
    DevBuf<uint8_t> bgr_all;    // [C][H*W*3] the images of vc_foreground_to_slot as copied (one staged copy for all cameras)
    Pinned<uint8_t> h_bgr_all;
    DevBuf<uint32_t> bits;      // [C][mwords]
    DevBuf<uint32_t> frames;    // [C][H*W] one dword per pixel: R | G << 8 | B << 16 | seen << 24 (a record's upper half)
    std::vector<uint8_t> have_frame, frame_dirty;
    bool have_masks = false;    // byte masks staged
    bool bits_valid = false;    // bits, record-layout images and the grid plan match the staged bytes
    bool grids_valid = false;   // block grids and camera order too (they also depend on grid, slab and cameras)
    DevBuf<uint32_t> grid;      // header + cropped block grids of all cameras (hierarchical kernels stage it in LDS)
    DevBuf<uint32_t> coarse;    // the same with 4 x 4 times coarser blocks, for the brick level (frame sets with large grids only)
    bool has_coarse = false;
    DevBuf<uint32_t> boxes;     // the cameras' foreground pixel boxes, two sets (see kBoxStride)
    uint32_t budget_words = 0;  // LDS budget the plan was made for (fixes the dynamic LDS size of the carve launch)
    uint32_t parity = 0;        // which of the header's two foreground-box sets the current frame filled
    bool counts_zero = false;   // the header's sample counts are zero (k_prep_pack just ran)
    Event e_up;                 // last upload into this slot (owned; upload stream)
    // The per-frame preparation runs on the UPLOAD stream, right behind the copy it works on and beside whatever the carve
    // stream is doing for the step before; e_prep (owned) marks its end, the carve waits for it.  e_p0: its start when timed.
    Event e_prep, e_p0;
    bool prep_pending = false, prep_timed = false;
    // borrowed from the step that used the slot last (recording an event between two kernels costs ~10 us of stream time,
    // so the slot rides on events a step records anyway): behind the last carve kernels that read the slot's bits / grids,
    // and behind the last record expansion that read its bits / images on the second stream.  The next preparation waits for both.
    hipEvent_t e_carve = nullptr, e_emit = nullptr;
    bool up_pending = false, carve_pending = false, emit_pending = false;
    uint32_t gen = 0;           // preparations so far: a step remembers the one it ran on (vc_carve_end's regrow path)
    DevBuf<uint32_t> sat;       // vc_carve_footprint: [C][(H+1)(W+1)] summed-area tables of `bits`, made by the first footprint carve
    uint32_t sat_gen = 0;       // ... that runs on a preparation of the slot, and the preparation they belong to
    bool sat_valid = false;
};

// np.linspace(lo, hi, num=n) in float64: y[k] = k*step + lo (two roundings), y[n-1] = hi
// (voxel_reconstruction.py:52-54).  Host code of this file is built contraction-free too.
void linspace(double lo, double hi, uint32_t n, std::vector<double> &out)
{
    out.resize(n);
    if (n == 0) return;
    if (n == 1) { out[0] = lo; return; }
    const double delta = hi - lo;
    const double div = (double)(n - 1);
    const double step = delta / div;
    for (uint32_t k = 0; k < n; ++k) {
        const double kk = (double)k;
        const double y = (step == 0.0) ? (kk / div) * delta : kk * step;
        out[k] = y + lo;
    }
    out[n - 1] = hi;
}

}  // namespace

// The route of one carve step: which kernels carve it, what they leave behind and what the stages behind them read.  Decided once per
// step (plan_route, settle_route), queued by step_carve, kept with the step for everything that comes later; DESIGN.md, section 4, has
// the table of families and conditions.  The families that stage a frame set's block grids in LDS come last (stages_grids).
enum class Carve : uint8_t { Foot, Generic, FusedChunked, LutStream, FusedHier, LutHier, Bricks };
enum class Table : uint8_t { None, YMajor, Tile, Color };    // Color: the colour camera's table over the whole grid (ensure_color_table)
struct StepRoute {
    Carve family = Carve::Generic;
    bool lut = false, viewmask = false;   // VC_MODE_LUT (Generic and Bricks come in both modes) | VC_FLAG_VIEWMASK (Foot, Generic)
    bool allseen = false;        // every survivor is seen by the colour camera: the threshold is C, or the footprint rule colours by the centre's pixel
    bool tile = false;           // FusedHier, LutHier, Bricks: words of 4 x-rows x 16 y (else y-lines)
    int boxes = 0;               // FusedHier: word boxes from float64 intervals (0), float32 intervals (1), read from ensure_boxes' (2)
    bool pair = false, b16 = false;   // LutHier on y-lines: two cameras per round trip; else (and LutStream) 16 alive words per batch, not 8
    bool boxed_tiles = false;    // tile words whose boxes are read: the routes the brick boxes serve (Bricks where brick_shape holds, else k_cull)
    bool cull = false;           // k_cull runs in front of the one-launch kernel
    bool zero_counts = false;    // waves and groups do not coincide (!tile_whole): counts by atomics into zeroed memory, every word stored
    bool counted = false, sparse_words = false;   // the kernels leave the group counts (else k_count_groups) | and dead groups' words unwritten
    bool grids = false, wide_grids = false;       // the frame set's block grids are wanted | sized for the brick pipeline's LDS (148 KB, else 64)
    Table carve_table = Table::None, emit_table = Table::None;   // what the carve kernels | the record expansion look pixels up in
    bool try_lut16 = false, lut16 = false;        // the colour camera's compact table may be tried | is what the expansion reads (ensure_lut16)
    bool count_nz = false;       // k_assemble counts the groups' non-zero words for the packing (StepBuf::nz_valid starts from this)
    bool busy = false;           // the scan lists the groups with survivors (k_finish_scan); expansion and packing stride over the list
    size_t lds = 0;              // dynamic LDS of the carve kernels (stages_grids: known once the frame set is prepared)
    // the step's events: a rank packs and exchanges its counts behind the scan | on another stream than the carve's; {scan done} is
    // wanted | rides on k_finish_scan; {expansion begun, step done} ride on the expansion
    bool exchange = false, xstream = false, scan_ev = false, scan_ridden = false, ride = false;
};

// One carve step's device state.  Two of them exist so that step i+1 can be enqueued before the
// host has collected step i (vc_carve_begin / vc_carve_end): the device never idles between steps.
struct StepBuf {
    StepRoute route;
    DevBuf<uint64_t> words;
    DevBuf<uint32_t> groupcnt, groupoff;
    DevBuf<uint32_t> groupnz;                // non-zero words per group (brick pipeline, compact exchange: k_assemble counts them in passing)
    bool nz_valid = false;
    DevBuf<uint64_t> blocksum, blockoff;     // blockoff[nscan] = total
    DevBuf<uint64_t> records;
    Pinned<uint64_t> h_total;                // one scalar
    Event e0, e_first, e1, e_prep;
    hipEvent_t e2 = nullptr, e_scan = nullptr, e_emit0 = nullptr;   // borrowed from vc_ctx::step_ev for the step in this set (see there)
    bool emit_ridden = false;                // e_emit0 / e2 are the expansion launch's own begin and end
    // option timing_detail: begin / end events of this step's kernels by kind (owned, made on first use; they ride on the launches),
    // which pair each kind used (the expansion and k_finish_scan may carry the step's own events instead), and which kinds ran
    Event kev[VC_KERNEL_KINDS][2];
    hipEvent_t kused[VC_KERNEL_KINDS][2] = {};
    uint32_t kmask = 0;
    bool prepped = false, prep_timed = false; // this step queued preparation kernels in front of its carve (timed: e_prep .. e0)
    bool carve_timed = false;                // e0 / e1 were recorded around the carve kernels (synchronous calls, timing_detail)
    bool emit_timed = false;                 // e_scan / e2 bracket the record expansion
    bool pending = false, used = false;
    EmitParams emit;                         // kept for a re-run after a records regrow
    bool no_records = false;                 // VC_FLAG_NO_RECORDS: occupancy words + count only
    bool sparse_words = false;               // words of groups with groupcnt == 0 were left unwritten
    DevBuf<uint32_t> busyoff, busysum, busyblock, busylist;   // the groups with survivors, listed by the scan (route.busy)
    // compact exchange form of this step: non-zero words as {bits, global index of bit 0} pairs
    DevBuf<uint64_t> ent, mine, counts;      // pairs | {entries, survivors} of this rank | of all ranks
    Pinned<uint64_t> h_counts;               // 2 per rank
    bool counts_exchanged = false;           // vc_carve_begin already packed and all-gathered the counts
    int color_cam = -1;                      // what the step was run with (vc_expand_entries colours the same way; the mode: route.lut)
    uint32_t slot = 0, slot_gen = 0;         // frame set the step read, and which preparation of it
    uint32_t min_views = 1;                  // the threshold it ran with, after the clamp to >= 1 (vc_surface_mesh's point test)
    uint64_t n = 0, survivors = 0;
};

constexpr int kDepth = 3;                   // sets of result buffers = carve steps that may be in flight: with two, the host cannot queue step i + 1
                                            // before it has collected step i - 1, whose expansion ends when the carve of step i does -- the carve
                                            // stream then idles for the host's round trip (20 us of a 155 us step)
constexpr uint32_t kStepRing = 64;
constexpr uint64_t kNever = 0;              // the stamp of a product that was never made, or was dropped (vc_ctx::result_gen starts above it)
constexpr uint32_t kGatherRing = 32;        // steps before a gather's events are recorded again (more than the resident frame sets a stream cycles through)
struct vc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // scan + record expansion of step i, beside the carve of step i+1 on `stream`
    hipStream_t stream_up = nullptr; // host-to-device copies of masks and images (overlap the carve in flight)
    hipStream_t stream_x = nullptr;  // a rank of a communicator: packing + collectives of step i, beside the carve of step i + 1 (they waited in
                                     // line on the carve stream: three launches, two collectives and their events, ~60 us per step)
    Event ev_h[2];                   // around the last mask upload (h2d_ms)
    bool h2d_pending = false;
    int overlap = 1;                 // (one stream when a communicator is attached: its collectives order everything)
    // How the streams share the chip.  The record expansion fills every wave slot (65 536 waves of streaming work); the carve
    // chain is a row of short, latency-bound launches that then queue for slots behind it.  stream_priority: carve + preparation
    // streams at the highest queue priority, the expansion stream at the lowest -- the dispatcher hands a freed slot to the
    // carve chain first.  reserve_cus: k compute units per XCD (k x 8 of 256) are left out of the expansion stream's CU mask
    // (hipExtStreamCreateWithCUMask; no priority then: that call has none), so the carve chain always finds free slots there.
    int stream_priority = 1;
    int reserve_cus = 0;
    int launch_events = 1;           // the events the streams exchange ride on the launch that precedes them (hipExtLaunchKernelGGL's stop event: the
                                     // kernel's own completion signal) instead of a barrier packet of their own behind it (~3.5 us of stream time each)
    int event_scope = 1;             // 1: the events the streams exchange release to the DEVICE only (no system-scope write-back)
    StepBuf sb[kDepth];
    int head = 0, npending = 0, cur = -1;    // next set to issue into, steps in flight, set holding the fetched result
    Event ev[4];
    // the compact all-gather's events {start, expansion done, payload arrived}, a RING of them: a frame set's next preparation
    // waits for the expansion that read it (Slot::e_emit), many steps later -- one event re-recorded every step would make it
    // wait for the newest expansion instead and put carve, exchange, expansion and preparation in one line
    Event gx[kGatherRing][3];
    // the same for a step's {scan done, step done}: frame sets remember them (Slot::e_carve, e_emit) for their next preparation,
    // kStepRing steps of distance keep that wait on the step that read the frame set and not on a newer one
    Event step_ev[kStepRing][3];                // {scan done, step done, expansion begun}
    uint32_t step_next = 0;
    uint32_t gx_next = 0;
    std::string err;

    // grid
    uint32_t nx = 0, ny = 0, nz = 0, z0 = 0, z1 = 0;
    double bounds[6] = {0, 0, 0, 0, 0, 0};
    std::vector<double> xs, ys, zs;
    DevBuf<double> d_axes;           // xs | ys | zs
    bool have_grid = false;

    // cameras
    uint32_t C = 0, H = 0, W = 0, mwords = 0;
    CamDev cams[VC_MAX_CAMERAS];
    bool have_cams = false;

    std::vector<Slot> slots;
    uint8_t post_open[VC_MAX_CAMERAS] = {0}, post_close[VC_MAX_CAMERAS] = {0};   // 2x2 open / close per camera
    DevBuf<uint8_t> d_morph;         // post-filtered byte masks [C][H*W] + one scratch image

    DevBuf<int32_t> d_lut;
    DevBuf<uint64_t> d_bbox;         // [C][n_pad/64] per-word pixel boxes (built with the LUT)
    DevBuf<int32_t> d_lut_tile;      // the table in tile order (words of 4 x-rows x 16 y), when the grid allows
    DevBuf<uint64_t> d_tbox;         // pixel boxes of the tile words
    DevBuf<uint64_t> d_kbox;         // pixel boxes of the 16^3 bricks (64 tile words each)
    DevBuf<uint64_t> d_live;         // per frame set: bit per brick "may hold survivors" | "all voxels survive" (k_cull)
    // brick pipeline (k_cull_bricks -> k_brick_words -> k_voxel_words -> k_assemble)
    DevBuf<uint64_t> d_wbox;         // [C][nbrick_pad * 64] brick-major word boxes (geometry only)
    DevBuf<uint64_t> d_bm;           // [n_pad / 64] tile-word results of the current step, tile order
    DevBuf<uint32_t> d_blist;        // counters [8] | brick list [nbrick_pad] | column list
    DevBuf<uint64_t> d_wlist;        // undecided words (worst case: every word of the slab)
    Pinned<uint32_t> h_lists;        // [4]: list lengths of an earlier step, to size launches by
    // marching cubes (vc_marching_cubes)
    DevBuf<uint64_t> d_mcbits, d_mcx;
    DevBuf<uint32_t> d_mcwbase, d_mcfaces;
    ScanBufs d_mcv, d_mct;           // scans of the vertex and triangle counts per group
    DevBuf<float> d_mcverts;
    uint64_t mc_verts = 0, mc_faces = 0;
    bool mc_valid = false;
    uint32_t list_parity = 0;
    uint32_t cull_probe = 0;         // steps that skipped the brick-level tests (launch_bricks: every 64th looks again)
    int bricks = 1;                  // the brick pipeline where the grid shape allows (ny in {256, 512, 1024})
    int dbg = 0;
    bool big_lds_ok = false;
    int voxel_batches = 0;                   // k_voxel_words: batches of 8 words a wave takes one after the other; 0 = by kernel form (launch_bricks)
    int voxel_pairs = 0;                     // k_voxel_words: 0 = by camera count, 1 = two cameras per round, 2 = one
    bool kbox_valid = false;
    int cull = 1;                    // hierarchical kernels on tile words: cull whole bricks first
    bool tile_valid = false;
    bool bbox_valid = false, tbox_valid = false;   // boxes match the grid, slab and cameras (also built without a table)
    int grid_lds_kb = 0;             // LDS budget of a frame set's block grids (picks their resolution); 0 = by frame-set size (16 or 64)
    int grid_min_shift = 1;          // finest block: 2^shift pixels
    int lut_tile = 1;                // hierarchical LUT kernel on tile words (needs nx % 4 == 0, ny % 64 == 0)
    int fused_tile = 1;              // the same word shape for the hierarchical table-free kernel
    int fused_f32box = 1;            // its word boxes from float32 intervals after a float64 rigid transform ...
    int fused_color_table = 1;       // VC_MODE_FUSED: colour the survivors from the colour camera's table (one camera, whole grid; 0: project each survivor again)
    int fused_boxes = 1;             // ... or read from boxes reduced once from the exact pixels (no table involved)
    bool lut_valid = false;          // vc_build_lut ran for this grid / slab / cameras (tile-ordered table, or y-major where tiles do not apply)
    uint32_t upload_mask = 0;        // cameras handed in by vc_upload_lut so far
    bool lut_foreign = false;        // the table in use came in through vc_upload_lut
    bool ymajor_valid = false;       // the y-major table + y-line boxes exist (built on demand: streaming / generic kernels, vc_fetch_lut)
    // tuning knobs (vc_set_option); defaults are the measured best on MI355X
    bool force_generic = false;      // one-thread-per-voxel kernels only (cross-check path)
    int first_kv = 1;                // dwordx4 loads per lane per chunk in k_lut_first: 1, 2 or 4
    int first_blocks_per_cu = 3;     // k_lut_first workgroups (512 threads) per CU
    int refine_b = 8;                // alive words per batch in k_lut_refine: 8 or 16
    int refine_blocks_per_cu = 8;    // k_lut_refine workgroups (256 threads) per CU
    int fused_blocks_per_cu = 8;     // k_carve_fused workgroups (256 threads) per CU
    int reorder = 1;                 // visit the most selective camera first
    int hier_blocks_per_cu = 48;     // hierarchical kernel: oversubscribed grid, the dispatcher balances uneven groups
    int refine_pair = 1;             // hierarchical LUT kernel: two cameras per dependent round trip
    int emit_lanes = 1;              // record expansion: lanes = voxels of a word (1) or lanes = survivors (0)
    int emit_busy = 1;               // ... driven by the list of busy groups (grids of >= kBusyListMinGroups groups)
    int emit_waves_per_cu = 256;     // waves of that launch per CU (a wave strides over the list when there are more busy groups)
    // The colour camera's tile-ordered table in compact form (k_pack_lut16: 2 B per entry + 4 B per tile word), what the
    // expansion of VC_MODE_LUT reads instead of d_lut_tile where it fits: one camera at a time, packed by the first step that
    // names the camera (ensure_lut16), void with d_lut_tile (drop_lut16)
    int emit_lut16 = 1;
    DevBuf<uint16_t> d_lut16;
    DevBuf<int32_t> d_cbase;
    DevBuf<uint32_t> d_lut16_flag;
    int lut16_cam = -1;              // the camera d_lut16 holds (-1: none)
    uint32_t lut16_nofit = 0;        // cameras whose table does not fit 16 bits (or found no memory): 4-byte entries, not tried again
    bool last_emit16 = false;        // the expansion launched last read the compact table (vc_debug_counters)
    int fused_hier = 1;              // VC_MODE_FUSED: interval-arithmetic word rejection (needs ny % 64 == 0)
    int lut_hier = 1;                // VC_MODE_LUT: hierarchical kernel (boxes + block grid) instead of stream + refine
    int timing_detail = 0;           // also time preparation and carve kernels of pipelined steps (three more events on the carve stream)
    int kernel_events = 0;           // every launch of a step carries begin / end events of its own (no packet of their own: vc_timing_t::kernel_ms_sum)
    DevBuf<double> d_foot_axes;      // the cell lattices lx | ly | lz (nx + 1, ny + 1, nz + 1 values), made by the first footprint carve on a grid
    bool foot_axes_valid = false;
    DevBuf<uint16_t> d_viewmask;
    DevBuf<double> d_scratch;
    Pinned<uint64_t> h_total;        // one scalar (all-gather count)
    bool viewmask_valid = false, carved = false;
    uint64_t survivors = 0;
    // The generation of the current result.  Whatever changes the records or the occupancy advances it (result_changed); a product
    // of a post-carve pass keeps the generation it was made on as its stamp and is valid / current while the two are equal.  A pass
    // sets its own stamp to kNever when it starts and to result_gen when it has finished, and touches nobody else's.
    uint64_t result_gen = 1;
    bool current(uint64_t stamp) const { return stamp == result_gen; }
    // Scratch the passes over the result share, one after the other on the context's stream.  h_res holds each pass's own read-backs
    // (photo: [0] removal count of the round, low 32 bits, [1] compaction total; components: [0] components, [1] kept records, [2] misc)
    ScanBufs d_rscan;                // scans of the compactions (photo, components, morphology) and of word_offsets (components, grow, temporal, normals, geodesic)
    DevBuf<uint32_t> d_woff;         // survivors before each occupancy word (word_offsets), good for the pass that made it only: components, grow, temporal, normals
    DevBuf<uint64_t> d_rec_spare;    // the records' second buffer: a compaction's or a merge's target, then swapped with the step's
    Pinned<uint64_t> h_res;          // three pinned scalars (pass_begin makes them)
    std::vector<Event> dist_ev;      // timing_detail: begin / end events of the launches of distance, morphology, grow and geodesic (VC_DLAUNCH), made on first use
    std::vector<int> dist_ev_kind;   // the kernel kind of each pair the running call has used
    // What each pass over the result keeps: its buffers, its stamp (see result_gen), its counts, its options.
    // vc_color_visible: depth maps [C][H W] (float32 bits), camera mask per survivor, surface list + counters, large-rectangle queue
    struct Visible {
        DevBuf<uint32_t> zmap, list, ctr;
        DevBuf<uint16_t> mask;
        DevBuf<uint4> queue;
        uint64_t stamp = kNever;         // the maps and masks belong to the current carve result
        int check = 1;                   // splats look at the stored depth before their atomic
        int big_rect = 64;               // pixels above which a splat rectangle gets a workgroup of its own
    } visible;
    // vc_photo_carve: round per input record, removal counter per round
    struct Photo {
        DevBuf<uint8_t> rounds;
        DevBuf<uint32_t> removed;
        uint64_t stamp = kNever;         // rounds belongs to the photo carve that produced the current result
        uint64_t n = 0;                  // its input survivors
    } photo;
    // vc_hull_components: the union-find forest, labels, component numbers of the roots, the root list, sizes, boxes, keep flags,
    // component entries, [kept components, largest], the select threshold (the survivors before each word: vc_ctx::d_woff)
    struct Components {
        DevBuf<uint32_t> parent, label, cid, roots, size, box, comp, misc;
        DevBuf<uint8_t> kept;
        DevBuf<uint64_t> thr;
        uint64_t stamp = kNever;         // labels and components belong to the pass that produced the current result
        uint64_t n = 0;                  // its input survivors
        uint32_t k = 0;                  // its components
    } components;
    // vc_hull_distance and vc_hull_morphology: the inside field over the hull's box, the outside field over the grid, the other
    // field of an envelope pass, the envelope stacks, the records' values, the survivors' box, [max, records above r2] x 2
    struct Distance {
        DevBuf<uint64_t> in, out, tmp, rec;
        DevBuf<uint32_t> st, d_box;
        DevBuf<unsigned long long> acc;
        uint64_t stamp = kNever;         // the fields belong to the vc_hull_distance that ran on the current result
        bool outside = false;            // ... with VC_DIST_OUTSIDE
        uint64_t n = 0;                  // its survivors
        DistBox box = {};                // the box of `in`
        uint64_t work[2] = {0, 0};       // VC_WORK_DIST_CELLS, VC_WORK_DIST_LINES since vc_timing_reset
    } distance;
    // vc_hull_grow: the added bits of the word range its box spans, [added, |Dl|], the `added` byte of each record
    struct Grow {
        DevBuf<unsigned long long> addw, ctr;
        DevBuf<uint8_t> added;
        uint64_t stamp = kNever;         // added belongs to the vc_hull_grow that produced the current result
        uint64_t n = 0;                  // its survivors_after
    } grow;
    // vc_hull_motion / vc_hull_warp / vc_paint_motion: voxel counts per block, the groups' masks of listed blocks, the rows, the
    // vector of each block, the counters and their read-back; the launch geometry of the field and the register it was made against
    struct Motion {
        DevBuf<uint32_t> counts, vec;
        DevBuf<uint64_t> mask;
        DevBuf<MotionRow> rows;
        DevBuf<unsigned long long> ctr;
        Pinned<uint64_t> h;              // page-locked read-back of the counters
        MotionGrid g = {};
        uint64_t stamp = kNever;         // the field belongs to the vc_hull_motion that ran on the current result ...
        uint32_t reg = 0;                // ... against this register, which has not been written since (motion_reg_written)
        uint64_t listed = 0;
        uint32_t levels = 0, refine = 0; // the coarser levels and the refine radius of the call that made it (vc_hull_motion: 0, 0) ...
        uint32_t reach = 0;              // ... and the largest component its vectors can have (vc_hull_motion: the search range)
    };
    // vc_hull_motion_pyramid: the coarser levels 1..3 of the field in `motion` (level l in level[l - 1]: its blocks, rows, vectors
    // and counters, with its grid and listed blocks), and their occupancy words of A and of B.  Current while `motion` is.
    struct Pyramid {
        Motion level[3];
        DevBuf<uint64_t> wa[3], wb[3];
    } pyramid;
    // vc_hull_temporal: the ring of the last `window` hulls ([window][npad] words, slot `head` the newest), the previous output P,
    // the staging buffer of O_t (swapped with P by a finished call), the five counters and their read-back, the records' vote and
    // `added` bytes.  Ring, P, window, head and pushes OUTLIVE a result: a carve leaves them alone, geometry_changed starts them over.
    // vc_hull_temporal_motion shares all of it and adds the second ring its aligned snapshots are written to (swapped with the first
    // by a finished call), the kind of call that filled the ring, and a field of its own (its stamp and register are not used:
    // the field is current while `stamp` below is).
    struct Temporal {
        DevBuf<uint64_t> ring, prev, stage;
        DevBuf<uint64_t> ring2;          // vc_hull_temporal_motion only
        bool aligned = false;            // the ring was filled by vc_hull_temporal_motion: a call of the other kind starts it over
        bool has_field = false;          // ... and the call that produced the current result was one (vc_fetch_temporal_motion)
        Motion field;
        DevBuf<unsigned long long> ctr;
        Pinned<uint64_t> h;              // page-locked read-back of the counters
        DevBuf<uint8_t> votes, added;
        uint64_t stamp = kNever;         // votes and added belong to the vc_hull_temporal that produced the current result
        uint64_t n = 0;                  // its survivors_after
        uint32_t window = 0, head = 0;   // the ring's length, the slot of the newest snapshot
        uint64_t pushes = 0;             // calls since the last reset (0: ring and P are empty)
        uint64_t nwords = 0, npad = 0;   // occupancy words of a snapshot, and the even count its slot holds
    } temporal;
    // vc_hull_keep / vc_hull_upload / vc_hull_combine / vc_hull_compare: the kept hulls (occupancy words [npad] with a zeroed pad, the
    // voxel count, optionally the records), the staging buffer of R (after a commit that added voxels: A's words), the counters
    // and their read-back, the records' `added` bytes; the comparison's own box field, index boxes and maxima.  The registers
    // OUTLIVE a result: a carve leaves them alone, geometry_changed empties them.
    struct Kept {
        DevBuf<uint64_t> words, rec;
        uint64_t count = 0;
        bool used = false, has_rec = false;
    };
    struct Setops {
        Kept reg[VC_HULL_REGISTERS];
        DevBuf<uint64_t> stage, field;
        DevBuf<unsigned long long> ctr, acc;
        DevBuf<uint32_t> box;
        Pinned<uint64_t> h;              // page-locked read-back of counters, boxes and maxima
        DevBuf<uint8_t> added;
        uint64_t stamp = kNever;         // added belongs to the vc_hull_combine that produced the current result
        uint64_t n = 0;                  // its survivors_after
    } setops;
    Motion motion;
    // vc_render: the images of the last render ([V][H W] index, depth, colour | face << 24), its views, the block map, counters
    struct Render {
        DevBuf<uint32_t> idx, rgbf;
        DevBuf<float> depth;
        DevBuf<RenderView> views;
        DevBuf<uint64_t> map;
        DevBuf<unsigned long long> ctr;
        bool valid = false;              // images of a finished render (a new carve leaves them alone)
        uint64_t stamp = kNever;         // the images of the last render show the current result (valid outlives a carve)
        uint32_t n_views = 0, H = 0, W = 0;
        int blocks = 1;                  // vc_render skips empty 8^3 blocks (same results)
        bool map_built = false;          // the last render filled the block map (vc_light_render walks with it)
    } render;
    // vc_surface_mesh: edge entries, the mesh of the last call (world vertices, faces, colours, refined flags), counters
    struct Surface {
        DevBuf<uint64_t> edges;
        DevBuf<double> verts;
        DevBuf<uint32_t> faces;
        DevBuf<uint8_t> rgb, refined;
        DevBuf<unsigned long long> ctr;
        uint64_t n_verts = 0, n_faces = 0;
        bool valid = false;
        uint64_t stamp = kNever;         // the last surface mesh was made on the current result (valid outlives a carve)
        int order = 1;                   // vc_surface_mesh tries the cameras that rejected P_off first (same results)
    } surface;
    // vc_hull_normals: the ball's rows, the records' quadruples, [surface, zero]; the shaded images of
    // vc_shade_render ([V][H W] R | G << 8 | B << 16) and its lights; the quadruples of the last mesh's vertices
    struct Normals {
        DevBuf<uint32_t> rows, sh_rgb;
        DevBuf<short4> out, verts;
        DevBuf<unsigned long long> ctr;
        DevBuf<double> sh_light;
        uint64_t stamp = kNever;         // the quadruples belong to the vc_hull_normals that ran on the current result
        uint64_t n = 0;                  // its survivors
        bool sh_valid = false;           // shaded images of the last render exist
    } normals;
    // vc_texture_render: the textured images of the last render ([V][H W] R | G << 8 | B << 16 | count << 24, the refined depth,
    // the heaviest camera, the refined flag), [hits, refined, textured, fallback, camera tests] and their read-back
    struct Texture {
        DevBuf<uint32_t> rgbc;
        DevBuf<float> depth;
        DevBuf<uint8_t> best, refined;
        DevBuf<unsigned long long> ctr;
        Pinned<uint64_t> h;              // page-locked read-back of the counters
        bool valid = false;              // textured images of the last render exist
    } texture;
    // vc_light_render: the lit images of the last render ([V][H W] R | G << 8 | B << 16, depth, kind, shadow, ao), the list of the
    // pixels that cast rays, [hull, floor, shadowed, facing away, rays, cells looked at, blocks skipped] and their read-back
    struct Light {
        DevBuf<uint32_t> rgb, jobs;
        DevBuf<float> depth;
        DevBuf<uint8_t> kind, shadow, ao;
        DevBuf<unsigned long long> ctr;
        Pinned<uint64_t> h;              // page-locked read-back of the counters
        bool valid = false;              // lit images of the last render exist
    } light;
    // vc_hull_clusters: survivors per column, the columns' and the records' labels, the histograms [K][512], the boxes [K][6],
    // the accumulators (kClAccTotal u64, layout at vc_hull_clusters), the seeds' columns; the clusters as the host assembled them
    struct Clusters {
        DevBuf<uint32_t> fmap, hist, box, seed;
        DevBuf<uint8_t> flab, lab;
        DevBuf<unsigned long long> acc;
        Pinned<uint64_t> h;              // page-locked read-back of the accumulators
        std::vector<vc_cluster_t> out;
        uint64_t stamp = kNever;         // labels, clusters and maps belong to the vc_hull_clusters that ran on the current result
        uint64_t n = 0;                  // its survivors
        uint32_t k = 0, ncol = 0;        // its K and nx ny
        int floor_records = 1;           // the floor map by one atomic per record (measured the faster way); 0: from the occupancy words
    } clusters;
    // vc_hull_geodesic: a key per record, the words' record offsets, the tile lists and their flags (two parities), the counters
    // (kGeoCnt* u32), the accumulators (kGeoAcc* u64), the seeds as given, a path; what the host keeps of the last call
    struct Geodesic {
        DevBuf<unsigned long long> key, acc;
        DevBuf<uint32_t> woff, flag, list, cnt, seeds, path;
        Pinned<uint64_t> h;              // page-locked read-back of counters and accumulators
        std::vector<vc_extremum_t> ext;
        std::vector<std::vector<uint32_t>> paths;   // [extremities] with VC_GEO_PATHS, else empty
        GeoParams p = {};                // the launch parameters of the last call (vc_geodesic_path walks with them)
        uint64_t stamp = kNever;         // keys and extremities belong to the vc_hull_geodesic that ran on the current result
        uint64_t n = 0, max_d = 0;       // its survivors and stats.max_d
        uint32_t conn = 0;               // its connectivity
        int tiles = 1;                   // the relaxation by tiles in LDS; 0: by sweeps over all records (the same bytes)
    } geodesic;
    // vc_hull_measure: the G output structs, the host's labels on the device, the profile [G][nz][3], the workgroups' tables
    // [workgroups][min(G, kMsTable)] before k_ms_fold adds them up; the structs as read back
    struct Measure {
        DevBuf<unsigned long long> out, prof, part;
        DevBuf<uint32_t> lab;
        Pinned<uint64_t> h;              // page-locked read-back of the structs
        uint64_t stamp = kNever;         // the structs and the profile belong to the vc_hull_measure that ran on the current result
        uint32_t g = 0, nz = 0;          // its G and the layers of its profile
        bool profile = false;            // ... which it made (VC_MEASURE_PROFILE)
    } measure;
    // vc_hull_thin: the working copy of the occupancy, the anchors' bits and the bits of the voxels the border list has held, the
    // border list (two buffers, compacted from one into the other once per pass; the kept voxels at the end), a direction step's
    // candidates, the words' record offsets, peel per record, the skeleton's rows, the counters (kThCnt*), the host's anchors on
    // the device, the predicate's table (built once per context)
    struct Thin {
        DevBuf<unsigned long long> work, anchor, listed, live[2], cand;
        DevBuf<uint32_t> woff;
        DevBuf<uint16_t> peel;
        DevBuf<ThRow> rows;
        DevBuf<uint32_t> cnt, list, table;
        Pinned<uint32_t> h;              // page-locked read-back of the counters
        uint64_t stamp = kNever;         // peel and rows belong to the vc_hull_thin that ran on the current result
        uint64_t n = 0, kept = 0;        // its survivors and its kept voxels
        bool table_built = false;
        int use_table = 0;               // option thin_table: the predicate by look-up; 0: in registers (the same bytes)
    } thin;
    // vc_hull_shell: the level-0 face byte per record, the shell's records and face bytes, the coarse occupancy and its shell
    // words with the cells of the list before each (levels above 0), the colour accumulators [T][4], the counters (kShCounters);
    // the viewer's tables and arrays (vc_fetch_shell_viewer)
    struct Shell {
        DevBuf<uint8_t> fb, faces;
        DevBuf<uint64_t> rec, cwords, shw;
        DevBuf<uint32_t> woff, acc;
        DevBuf<unsigned long long> cnt;
        DevBuf<float> tab, view;
        Pinned<uint64_t> h;              // page-locked read-back of the counters
        uint64_t stamp = kNever;         // the list belongs to the vc_hull_shell that ran on the current result
        uint64_t T = 0;                  // its shell cells
        uint32_t level = 0, dims[3] = {0, 0, 0};   // its level and (coarse) grid
    } shell;

    // comm
    ncclComm_t comm = nullptr;
    int n_ranks = 1, rank = 0;
    DevBuf<uint64_t> d_counts, d_gathered;
    Pinned<uint64_t> h_counts;       // n_ranks
    uint64_t gathered_total = 0;
    bool gathered = false;
    // compact exchange: non-zero words of the slab as {bits, global index of bit 0} pairs
    int gather_compact = 1;          // vc_allgather exchanges the pairs and expands them on every rank
    int gather_sync = 1;             // 0: vc_allgather returns once its work is queued (count known from the ranks' counts)
    // Two compact gathers may be in flight (gather_sync 0): gather k uses half k & 1 of what follows -- its payload buffer
    // (all ranks' pairs in rank order: the next payload arrives while the expansion of this one still reads it), its events, its
    // expected total.  The records go to the one d_gathered: expansions are in order on their stream and a read-back ends them.
    bool gpend[2] = {false, false};  // a queued all-gather whose completion has not been observed yet
    uint32_t gx_idx[2] = {0, 0};
    uint64_t gexpect[2] = {0, 0};
    uint32_t gseq = 0;               // compact gathers issued
    DevBuf<uint64_t> d_ent_all[2];
    ScanBufs d_xscan;                        // scan scratch of the pack pass ...
    ScanBufs d_yscan;                        // ... and of the expansion, which may run on the second stream beside a pack
    Pinned<uint64_t> h_xtotal;               // [4]
    uint64_t packed_entries = 0;
    bool packed = false;
    DevBuf<int32_t> d_lut_color;             // colour camera's table over the WHOLE grid (expansion of remote words)
    int lut_color_cam = -1;
    // One buffer, one camera at a time, yet steps in flight may name different colour cameras: {done} of the last expansion that
    // was handed the table on another stream than the carve stream (borrowed from step_ev / gx; null: none since the last
    // projection).  ensure_color_table makes the next camera's projection wait for it on the device.
    hipEvent_t lut_color_reader = nullptr;

    DevBuf<uint8_t> d_fg;            // vc_bgr_to_hsv / vc_mask_morphology: input | output | scratch images
    DevBuf<uint32_t> d_cc;           // vc_fill_figures / vc_foreground_to_slot: lab | own | tot | par planes per camera (vc_contour.h)
    DevBuf<int32_t> d_hsvdiv;        // OpenCV's two division tables of the 8-bit HSV conversion (sdiv | hdiv)
    struct MogModel {                // vc_mog_*: one background model (the reference keeps one per camera, assignment.py:79)
        bool used = false;
        int history = 200, nmixtures = 5;
        double background_ratio = 0.7, noise_sigma = 15.0;
        uint32_t H = 0, W = 0, nframes = 0;
        DevBuf<float> state;         // [8 nmixtures][H W] planes, see k_mog_apply
    } mog[VC_MAX_MOG_MODELS];
    struct Mog2Model {               // vc_mog2_*: one MOG2 background model, handle VC_MOG2_MODEL_TAG | index
        bool used = false;
        int history = 500, nmixtures = 5, shadow_value = 127;
        bool shadows = true;
        double var_threshold = 16;   // double((float)varThreshold), as OpenCV's constructor stores it
        float background_ratio = 0.9f, var_threshold_gen = 9.f, var_init = 15.f, var_min = 4.f, var_max = 75.f, ct = 0.05f, tau = 0.5f;
        uint32_t H = 0, W = 0, nframes = 0;
        DevBuf<float> state;         // [5 nmixtures][H W] planes, see k_mog2_apply
        DevBuf<uint8_t> nmodes;      // [H W]
    } mog2[VC_MAX_MOG_MODELS];
    vc_timing_t tm;
    StepBuf *kev_sb = nullptr;       // timing_detail: the step whose kernels are being queued (their launches carry its per-kind events)
    DevBuf<unsigned long long> d_stats;   // timing_detail: the kernels' work counters, [VC_WORK_KINDS][kShards][kStatStride]

    uint64_t n_voxels() const { return (uint64_t)nx * ny * (z1 - z0); }
    uint64_t i0() const { return (uint64_t)z0 * nx * ny; }
};

namespace {

int fail(vc_ctx *ctx, int code, const char *fmt, ...);

// The result is another from here on: every product of a post-carve pass is stale (their stamps no longer equal the generation).
void result_changed(vc_ctx *ctx) { ++ctx->result_gen; }

// The compact colour table is a copy of one camera of d_lut_tile: void, and its memory given back, whenever that table is
// built again or replaced (no step is in flight then, so nothing reads it).
void drop_lut16(vc_ctx *ctx)
{
    ctx->lut16_cam = -1; ctx->lut16_nofit = 0;
    ctx->d_lut16.reset(); ctx->d_cbase.reset();
}

// Grid, slab or cameras are others from here on: tables and boxes are to be built again, and there is no carve result.
void geometry_changed(vc_ctx *ctx)
{
    drop_lut16(ctx);
    ctx->lut_valid = false; ctx->upload_mask = 0; ctx->ymajor_valid = false; ctx->tile_valid = false; ctx->bbox_valid = false;
    ctx->tbox_valid = false; ctx->kbox_valid = false; ctx->carved = false; ctx->gathered = false; ctx->viewmask_valid = false;
    ctx->temporal.pushes = 0;                    // the hulls of another grid or other cameras are no history of this one
    for (vc_ctx::Kept &k : ctx->setops.reg) { k.used = false; k.has_rec = false; k.count = 0; }   // ... and no operands for it
    result_changed(ctx);
}

// (Re)creates an owned event with `flags`; page-locked host memory of at least `elems` elements (the "first use" allocations; a
// larger request replaces the block).
hipError_t make_event(Event &ev, unsigned flags = hipEventDefault)
{
    ev.reset();
    return hipEventCreateWithFlags(&ev.e, flags);
}

template <typename T>
hipError_t ensure_pinned(Pinned<T> &b, size_t elems)
{
    if (b.ptr && elems <= b.cap) return hipSuccess;
    b.reset();
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&b.ptr), elems * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) b.cap = elems;
    return e;
}

// timing_detail: the begin / end events launch `kind` of the step being queued is to carry (null otherwise: an ordinary launch)
void kev_pick(vc_ctx *ctx, int kind, hipEvent_t &start, hipEvent_t &stop)
{
    start = stop = nullptr;
    StepBuf *sb = ctx->kev_sb;
    if (!sb) return;
    for (int i = 0; i < 2; ++i)
        if (!sb->kev[kind][i] && make_event(sb->kev[kind][i]) != hipSuccess) return;
    start = sb->kev[kind][0]; stop = sb->kev[kind][1];
    sb->kused[kind][0] = start; sb->kused[kind][1] = stop;
    sb->kmask |= 1u << kind;
}
#define VC_KLAUNCH(kind, kernel, grid, block, lds, st, ...)                                             \
    do {                                                                                                \
        hipEvent_t ks_, ke_;                                                                            \
        kev_pick(ctx, kind, ks_, ke_);                                                                  \
        hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ks_, ke_, 0, __VA_ARGS__);                  \
    } while (0)

// (Re)creates the three streams for ctx->stream_priority / ctx->reserve_cus.  Nothing may be in flight.
hipError_t make_streams(vc_ctx *ctx)
{
    hipStream_t *all[4] = {&ctx->stream, &ctx->stream2, &ctx->stream_up, &ctx->stream_x};
    for (hipStream_t *st : all) {
        if (!*st) continue;
        hipError_t e = hipStreamSynchronize(*st);
        if (e == hipSuccess) e = hipStreamDestroy(*st);
        if (e != hipSuccess) return e;
        *st = nullptr;
    }
    int least = 0, greatest = 0;                                 // numerically: greatest priority <= least priority
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    const bool prio = ctx->stream_priority && least != greatest;
    if (ctx->reserve_cus > 0) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, ctx->device);
        if (e != hipSuccess) return e;
        // the driver deals the mask's bits round-robin over the XCDs (bit i -> XCD i % 8): the first 8 k bits are k compute
        // units of every XCD
        const uint32_t ncu = (uint32_t)prop.multiProcessorCount, words = (ncu + 31) / 32;
        const uint32_t reserved = (uint32_t)ctx->reserve_cus * 8u < ncu ? (uint32_t)ctx->reserve_cus * 8u : ncu / 2;
        std::vector<uint32_t> rest(words, 0u);
        for (uint32_t i = reserved; i < ncu; ++i) rest[i >> 5] |= 1u << (i & 31u);
        e = hipExtStreamCreateWithCUMask(&ctx->stream2, words, rest.data());
        if (e != hipSuccess) return e;
    } else {
        e = prio ? hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, least)
                 : hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
    }
    e = prio ? hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    e = prio ? hipStreamCreateWithPriority(&ctx->stream_up, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&ctx->stream_up, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    return prio ? hipStreamCreateWithPriority(&ctx->stream_x, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(&ctx->stream_x, hipStreamNonBlocking);
}

// The events that only order one stream behind another ({scan done} of a step: carve stream -> expansion stream; a frame set's
// {prepared}: upload stream -> carve stream) are recorded between two kernels of the critical path.  By default an event
// performs a SYSTEM-scope release when it is recorded (the host may want to look at what came before it): on this chip that is
// a write-back of every XCD's L2 -- with the expansion's 238 MB of records in flight beside it, ~12 us during which the recording
// stream stands still.  Nobody on the host ever looks at anything through these events: hipEventReleaseToDevice.  event_scope 2
// does the same to a step's {done} event, which the host DOES wait for (the survivor count it then reads sits in page-locked
// host memory, written past the caches).
hipError_t make_events(vc_ctx *ctx)
{
    ctx->lut_color_reader = nullptr;             // (borrowed from the ring made again below; everything has drained)
    for (uint32_t r = 0; r < kStepRing; ++r) {
        for (int i = 0; i < 3; ++i) {
            const bool dev = ctx->event_scope >= (i == 1 ? 2 : 1);
            hipError_t e = make_event(ctx->step_ev[r][i], dev ? hipEventReleaseToDevice : hipEventDefault);
            if (e != hipSuccess) return e;
        }
    }
    for (Slot &s : ctx->slots) {
        if (!s.e_prep) continue;
        hipError_t e = make_event(s.e_prep, ctx->event_scope >= 1 ? hipEventReleaseToDevice : hipEventDefault);
        if (e != hipSuccess) return e;
        s.prep_pending = s.carve_pending = s.emit_pending = false;   // (everything has drained: nothing to wait for)
    }
    return hipSuccess;
}

int fail(vc_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define VC_HIP(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(ctx, e_ == hipErrorOutOfMemory ? VC_ERR_OOM : VC_ERR_HIP, "%s: %s",    \
                        #call, hipGetErrorString(e_));                                         \
    } while (0)

#define VC_NCCL(ctx, call)                                                                     \
    do {                                                                                       \
        ncclResult_t r_ = (call);                                                              \
        if (r_ != ncclSuccess)                                                                 \
            return fail(ctx, VC_ERR_RCCL, "%s: %s", #call, g_rccl.GetErrorString(r_));         \
    } while (0)

template <typename T>
int ensure(vc_ctx *ctx, DevBuf<T> &b, size_t elems)
{
    if (elems <= b.cap && b.ptr) return VC_OK;
    b.reset();                                   // (the owner frees, vc_owned.h: as everywhere it does, an error of hipFree is dropped)
    if (elems == 0) elems = 1;
    VC_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&b.ptr), elems * sizeof(T)));
    b.cap = elems;
    return VC_OK;
}


#define VC_TRY(expr)              \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != VC_OK) return rc_; \
    } while (0)

uint32_t grid_for(uint64_t n);

void fill_params(const vc_ctx *ctx, CarveParams &p)
{
    memset(&p, 0, sizeof p);
    p.xs = ctx->d_axes.ptr;
    p.ys = p.xs + ctx->nx;
    p.zs = p.ys + ctx->ny;
    p.n = ctx->n_voxels();
    p.n_pad = (p.n + kLutPad - 1) / kLutPad * kLutPad;
    p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz; p.z0 = ctx->z0;
    p.C = ctx->C; p.H = ctx->H; p.W = ctx->W; p.mwords = ctx->mwords;
    memcpy(p.cam, ctx->cams, sizeof(CamDev) * ctx->C);
    p.bbox = ctx->d_bbox.ptr;
    p.lut_tile = ctx->d_lut_tile.ptr; p.tbox = ctx->d_tbox.ptr; p.tq = ctx->ny / 16;
    p.tile_whole = (p.tq != 0 && 64 % p.tq == 0) ? 1u : 0u;
    p.kbox = ctx->d_kbox.ptr;
    p.dbg = (uint32_t)ctx->dbg;
    p.live = nullptr;                                            // set by the launches that cull
    p.nbx = ((ctx->nx >> 2) + 3) / 4;
    p.nbz = (ctx->z1 - ctx->z0 + 15) / 16;
    p.nbrick_pad = (uint32_t)(((uint64_t)p.nbx * p.tq * p.nbz + 63) / 64 * 64);
}

constexpr int VC_MAX_RANKS = 64;
constexpr uint32_t kBusyListMinGroups = 16384;   // below 64 M voxels a wave per group is as fast and one launch shorter
constexpr uint32_t kMaxScanBlocks = 1024;  // 2^32 voxels / 4096 per group / 1024 groups per scan block
constexpr int kSub = 4;                    // 64-voxel sub-chunks per wavefront chunk (fused kernel)
constexpr size_t kLdsBytes = 160 * 1024;   // LDS per CU on gfx950
constexpr size_t kMaxFirstLds = 64 * 1024; // static limit of one workgroup's dynamic LDS without opt-in
constexpr size_t kWideGridBytes = 20 * 1024; // grids above this: 1024-thread workgroups share a copy, the brick level reads coarser blocks
constexpr size_t kMaxWideLds = 152 * 1024; // what the brick pipeline's grid-staging kernels may take (one 1024-thread workgroup per CU)
constexpr uint32_t kEstimateSamples = 1u << 16;

int ensure(vc_ctx *ctx, ScanBufs &b, uint32_t ngroups)
{
    VC_TRY(ensure(ctx, b.cnt, ngroups));
    VC_TRY(ensure(ctx, b.off, ngroups));
    VC_TRY(ensure(ctx, b.bsum, kMaxScanBlocks));
    VC_TRY(ensure(ctx, b.boff, kMaxScanBlocks + 1));
    return VC_OK;
}

// The bricks' pixel boxes and the brick-major copy of the word boxes (once per grid / slab / camera set, right behind the
// tile boxes).
int build_brick_boxes(vc_ctx *ctx)
{
    CarveParams p;
    fill_params(ctx, p);
    ctx->kbox_valid = false;
    if (p.nbrick_pad == 0) return VC_OK;
    VC_TRY(ensure(ctx, ctx->d_kbox, (size_t)p.nbrick_pad * ctx->C));
    VC_TRY(ensure(ctx, ctx->d_live, (size_t)(p.nbrick_pad / 64) * 2));
    VC_TRY(ensure(ctx, ctx->d_wbox, (size_t)p.nbrick_pad * 64 * ctx->C));
    p.kbox = ctx->d_kbox.ptr;
    hipLaunchKernelGGL(k_brick_boxes_bm, dim3(p.nbrick_pad / 4), dim3(kBlock), 0, ctx->stream, p, (const uint64_t *)ctx->d_tbox.ptr,
                       ctx->d_wbox.ptr, ctx->d_kbox.ptr);
    VC_HIP(ctx, hipGetLastError());
    ctx->kbox_valid = true;
    if (ctx->h_lists) ctx->h_lists[0] = ctx->h_lists[1] = ctx->h_lists[2] = 0xffffffffu;
    return VC_OK;
}

// Grid shapes the brick pipeline takes: a group of 4096 consecutive voxels must lie inside one brick column (see k_assemble).
bool brick_shape(const vc_ctx *ctx)
{
    if (!ctx->bricks || !ctx->cull || !ctx->kbox_valid) return false;
    if (ctx->ny != 256 && ctx->ny != 512 && ctx->ny != 1024 && ctx->ny != 2048 && ctx->ny != 4096) return false;
    if (ctx->nx % 4 != 0 || (ctx->ny < 1024 && ctx->nx % (4096u / ctx->ny) != 0)) return false;
    return true;
}

uint32_t sized(uint32_t known, uint64_t unknown_guess, uint64_t cap, uint32_t per_wg)
{
    uint64_t est = known == 0xffffffffu ? unknown_guess : (uint64_t)known + known / 4 + 64;
    if (est > cap) est = cap;
    uint64_t wgs = (est + per_wg - 1) / per_wg;
    if (wgs < 64) wgs = 64;
    if (wgs > 65536) wgs = 65536;
    return (uint32_t)wgs;
}

template <bool LUT>
int launch_bricks(vc_ctx *ctx, CarveParams &p, size_t lds, uint32_t ngroups)
{
    const uint32_t ncolumns = p.nbx * p.nbz;
    const uint32_t ipw = p.tq > 64 ? p.tq / 64 : 1;                           // rounds of 64 bricks per wave of k_cull_bricks (a whole column)
    const uint32_t nw = p.nbrick_pad / 64 / ipw;                              // waves of k_cull_bricks
    const uint32_t wps = (nw + kShards - 1) / kShards;                        // producers per shard
    BrickLists bl;
    bl.cap_b = wps * 64 * ipw; bl.cap_c = wps * 4;
    bl.cap_w = (p.nbrick_pad + kShards - 1) / kShards * 64;                   // a listed brick appends at most its 64 words
    VC_TRY(ensure(ctx, ctx->d_bm, (size_t)(p.n_pad / 64)));
    VC_TRY(ensure(ctx, ctx->d_wlist, (size_t)bl.cap_w * kShards));
    const size_t ncounters = 6 * (size_t)kShards * kShardStride;
    const size_t need = ncounters + (size_t)bl.cap_b * kShards + (size_t)bl.cap_c * kShards + 64;
    if (ctx->d_blist.cap < need) {
        VC_TRY(ensure(ctx, ctx->d_blist, need));
        VC_HIP(ctx, hipMemsetAsync(ctx->d_blist.ptr, 0, ncounters * sizeof(uint32_t), ctx->stream));    // both sets of list lengths
        ctx->list_parity = 0;
    }
    if (!ctx->h_lists) {
        VC_HIP(ctx, ensure_pinned(ctx->h_lists, 4));
        ctx->h_lists[0] = ctx->h_lists[1] = ctx->h_lists[2] = ctx->h_lists[3] = 0xffffffffu;       // unknown yet
    }
    bl.counters = ctx->d_blist.ptr;
    bl.bricks = ctx->d_blist.ptr + ncounters;
    bl.columns = bl.bricks + (size_t)bl.cap_b * kShards;
    bl.words = ctx->d_wlist.ptr;
    bl.bm = ctx->d_bm.ptr;
    bl.wbox = ctx->d_wbox.ptr;
    bl.host_counts = ctx->h_lists;
    bl.parity = (ctx->list_parity ^= 1u);
    p.live = ctx->d_live.ptr;
    const volatile uint32_t *known = ctx->h_lists;                // lengths of an earlier step (any size is correct: the waves stride)
    const uint32_t k_bricks = known[0], k_cols = known[1], k_words = known[2];
    // large grids (many cameras x large images): 16 waves share one LDS copy, so that the compute units stay full of waves
    // with two or three workgroups each; no more workgroups than fit the chip at once (they stride over the lists)
    const bool wide = lds > kWideGridBytes;
    const uint32_t wpg = wide ? kWideBlock / 64 : kBlock / 64;                // waves per workgroup
    const dim3 block(kBlock), gblock(wpg * 64);
    const uint32_t fit = 256u * (uint32_t)(kLdsBytes / (lds ? lds : 1) < 1 ? 1 : kLdsBytes / (lds ? lds : 1));
    const uint32_t lds_cap = wide ? fit : 65536u;
    const uint32_t cw = nw / wpg;
    uint32_t cull_wgs = cw < 1 ? 1 : (cw > 1024 ? 1024 : cw);
    if (cull_wgs > lds_cap) cull_wgs = lds_cap;
    uint32_t word_wgs = sized(k_bricks, p.nbrick_pad / 8, p.nbrick_pad, wpg);
    if (word_wgs > lds_cap) word_wgs = lds_cap;
    if (lds > kMaxFirstLds && !ctx->big_lds_ok) {                             // more than 64 KB of dynamic LDS is opt-in
        VC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cull_bricks), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxWideLds));
        VC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_brick_words_wide), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxWideLds + 6 * 1024)));
        ctx->big_lds_ok = true;
    }
    // Frame sets on which the brick level decides next to nothing (16 noisy cameras: every brick's box holds some foreground block
    // in every camera) pay its 35 us for nothing: when the earlier step whose list lengths are known listed at least nine bricks in ten,
    // this step lists them all without looking (the kernel stages no grids and tests no boxes; the word level decides them all the
    // same), and every 64th such step looks again.  Work only, never results.
    const uint32_t nbricks_all = p.nbx * p.tq * p.nbz;
    const bool cull_pays = k_bricks == 0xffffffffu || (uint64_t)k_bricks * 10u < (uint64_t)nbricks_all * 9u || (ctx->cull_probe++ & 63u) == 0u;
    if (!cull_pays || (ctx->dbg & 8192)) {
        p.cull_lds_words = 1;                                     // (nothing fits: nothing is staged)
        const uint32_t w4 = nw / (kBlock / 64);
        VC_KLAUNCH(VC_K_CULL_BRICKS, k_cull_bricks, dim3(w4 < 1 ? 1u : (w4 > 1024 ? 1024u : w4)), block, 64, ctx->stream, p, bl, ngroups);
        p.cull_lds_words = 0;
    }
    else if (wide && p.coarsegrid) {
        // the brick level reads the 4 x 4 times coarser grids (about a sixteenth of the words): no reason to share an LDS copy among 16
        // waves -- with nw / 16 workgroups it ran on 32 of the 256 compute units at 512^3.  Ordinary workgroups, as many as there are
        // wave loads of bricks; the bound on the coarse grids' length: a sixteenth of the fine ones + one more row and column per camera
        const size_t clds = ((size_t)(lds / sizeof(uint32_t)) / 8 + 64u * p.C + kGridHeader + 8) * sizeof(uint32_t);
        const uint32_t w4 = nw / (kBlock / 64);
        p.cull_lds_words = (uint32_t)((clds < lds ? clds : lds) / sizeof(uint32_t));      // (an estimate: the kernel checks it against the real length)
        VC_KLAUNCH(VC_K_CULL_BRICKS, k_cull_bricks, dim3(w4 < 1 ? 1u : (w4 > 1024 ? 1024u : w4)), block, clds < lds ? clds : lds, ctx->stream, p, bl, ngroups);
        p.cull_lds_words = 0;
    }
    else VC_KLAUNCH(VC_K_CULL_BRICKS, k_cull_bricks, dim3(cull_wgs), gblock, lds, ctx->stream, p, bl, ngroups);
    if (wide) {
        // + 1 KB per wave for the survivors' compaction (vc_kernels.h, brick_words_body) where the LDS has it: a camera mask and a lane number in 32 bits
        const size_t grid_words = (lds / sizeof(uint32_t) + 63u) & ~(size_t)63u;
        const size_t with = (grid_words + (kWideBlock / 64) * 256u) * sizeof(uint32_t);
        const bool compact = with <= kMaxWideLds + 6 * 1024 && p.C > 4 && p.C <= 23 && !(ctx->dbg & 16384);
        p.compact_off = compact ? (uint32_t)grid_words : 0u;
        VC_KLAUNCH(VC_K_BRICK_WORDS, k_brick_words_wide, dim3(word_wgs), gblock, compact ? with : lds, ctx->stream, p, bl);
        p.compact_off = 0;
    }
    else VC_KLAUNCH(VC_K_BRICK_WORDS, k_brick_words, dim3(word_wgs), gblock, lds, ctx->stream, p, bl);
    // many cameras: most voxels fail the first camera they ask, a second camera's entries read in the same round trip would be
    // wasted on them; few cameras: two per dependent round (the lists are short, the kernel is latency bound)
    const bool pairs = !LUT || ctx->voxel_pairs == 1 || (ctx->voxel_pairs == 0 && p.C <= 4);
    // batches a wave takes one after the other (the next one's entries under way): 8 where a batch is short (table look-ups, two cameras
    // per round: 0.1368 -> 0.1345 ms per step at 1024^3 x 4; 16: 0.147), 1 where it is long (projection 0.175 -> 0.19, one camera per round 0.30 -> 0.32)
    const uint32_t vb = ctx->voxel_batches ? (uint32_t)ctx->voxel_batches : (LUT && pairs ? 8u : 1u);
    const dim3 vgrid(sized(k_words, (uint64_t)p.nbrick_pad * 4, (uint64_t)p.nbrick_pad * 64, (pairs ? 32u : 64u) * vb));
    // one wave per workgroup for the two list-driven kernels that need no LDS: a workgroup of four has to find four free wave slots on one
    // compute unit at once, beside an expansion that refills every slot as it frees (the scans' lesson, in small: step -1.3 %)
    const uint32_t wpw = 1u;
    const dim3 vgrid2(vgrid.x * (4u / wpw)), sblock(64u * wpw);
    if (pairs) VC_KLAUNCH(VC_K_VOXEL_WORDS, (k_voxel_words<LUT, true>), vgrid2, sblock, 0, ctx->stream, p, bl);
    else VC_KLAUNCH(VC_K_VOXEL_WORDS, (k_voxel_words<LUT, false>), vgrid2, sblock, 0, ctx->stream, p, bl);
    VC_KLAUNCH(VC_K_ASSEMBLE, k_assemble, dim3(sized(k_cols == 0xffffffffu ? k_cols : k_cols * 16u, (uint64_t)ncolumns * 4, (uint64_t)ncolumns * 16, 4) * (4u / wpw)),
                       sblock, 0, ctx->stream, p, bl);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

int slot_at(vc_ctx *ctx, uint32_t slot, Slot **out)
{
    if (!ctx->have_cams) return fail(ctx, VC_ERR_ARG, "vc_set_cameras must precede frame uploads");
    if (slot >= 64) return fail(ctx, VC_ERR_ARG, "slot %u out of range (max 64 resident frame sets)", slot);
    if (slot >= ctx->slots.size()) ctx->slots.resize(slot + 1);
    Slot &s = ctx->slots[slot];
    if (s.have_frame.size() != ctx->C) { s.have_frame.assign(ctx->C, 0); s.frame_dirty.assign(ctx->C, 0); }
    if (!s.e_up) {
        VC_HIP(ctx, make_event(s.e_up, hipEventDisableTiming));
        VC_HIP(ctx, make_event(s.e_prep, ctx->event_scope >= 1 ? hipEventReleaseToDevice : hipEventDefault));
        VC_HIP(ctx, make_event(s.e_p0));
    }
    *out = &s;
    return VC_OK;
}

void release_slot(Slot &s)
{
    s.bytes.reset(); s.bits.reset(); s.frames.reset(); s.grid.reset(); s.coarse.reset(); s.boxes.reset();
    s.has_coarse = false;
    for (int c = 0; c < VC_MAX_CAMERAS; ++c) { s.fbytes[c].reset(); s.h_fbytes[c].reset(); }
    s.h_bytes.reset();
    s.bgr_all.reset(); s.sat.reset();
    s.sat_valid = false;
    s.h_bgr_all.reset();
    s.have_masks = s.bits_valid = s.grids_valid = false;
    s.have_frame.clear(); s.frame_dirty.clear();
}

// Queues, on the UPLOAD stream (behind the copy of the bytes it reads, beside the carve stream's work for the step before),
// whatever the slot's derived state is missing: bit masks + record-layout images + grid plan (k_prep_pack, after the optional 2x2
// post-filter), and for the chunked / hierarchical kernels the block grids and the camera order (k_prep_grid).  No host
// synchronisation: the kernels leave their results in the slot's header; e_prep marks their end for the carve stream.
int ensure_prepared(vc_ctx *ctx, Slot &s, bool want_grids, const CarveParams *cp, bool timed = false, bool wide_ok = false)
{
    const uint32_t C = ctx->C;
    const size_t HW = (size_t)ctx->H * ctx->W;
    hipStream_t st = ctx->stream_up;
    // grids made for the brick pipeline's 1024-thread workgroups do not fit the other kernels' LDS: prepare again
    if (want_grids && !wide_ok && s.bits_valid && (size_t)s.budget_words * sizeof(uint32_t) + 32 > kMaxFirstLds) s.bits_valid = s.grids_valid = false;
    if (s.bits_valid && !(want_grids && !s.grids_valid)) return VC_OK;
    // the kernels that still read what is about to be overwritten: carve kernels (bits, grids), record expansion (bits, images)
    if (s.carve_pending) { VC_HIP(ctx, hipStreamWaitEvent(st, s.e_carve, 0)); s.carve_pending = false; }
    if (s.emit_pending) { VC_HIP(ctx, hipStreamWaitEvent(st, s.e_emit, 0)); s.emit_pending = false; }
    s.prep_timed = timed;
    s.gen++;
    if (timed) VC_HIP(ctx, hipEventRecord(s.e_p0, st));
    if (!s.bits_valid) {
        VC_TRY(ensure(ctx, s.bits, (size_t)ctx->mwords * C));
        // LDS budget of header + grids: 16 KB (eight workgroups per CU) unless the frame set is so large that 16 KB would
        // force blocks of 32 x 32 pixels on it (16 cameras at 1080p).  The kernels that stage the grids are then launched
        // with few, persistent workgroups; the brick pipeline's run 1024 threads per workgroup, one or two per CU, so the
        // grids may take most of a CU's LDS (blocks of 8 x 8 pixels for 16 cameras at 1080p: masks with salt noise leave
        // 3 in 4 such blocks clean, 1 in 4 blocks of 16 x 16)
        const uint32_t cap_words = (uint32_t)((wide_ok ? 148u : 64u) * 256u);
        uint32_t budget = (uint32_t)ctx->grid_lds_kb * 256u;                  // u32 words of header + grids
        if (budget > cap_words) budget = cap_words;
        if (ctx->grid_lds_kb == 0) {
            budget = 16u * 256u;
            if ((uint64_t)ctx->mwords * C * 4 > (2u << 20)) {
                // what the UNCROPPED grids of all cameras take at the finest block that keeps them within the cap: cropping can
                // then only make the blocks finer, and the workgroups do not reserve more LDS than the grids can fill
                for (uint32_t sh = (uint32_t)ctx->grid_min_shift; sh < 15; ++sh) {
                    const uint64_t bw = ((uint64_t)ctx->W + (1u << sh) - 1) >> sh, bh = ((uint64_t)ctx->H + (1u << sh) - 1) >> sh;
                    const uint64_t total = kGridHeader + (uint64_t)C * 2 * ((bw + 31) / 32) * bh;
                    if (total <= cap_words || sh == 14) { budget = (uint32_t)(total < 16u * 256u ? 16u * 256u : total); break; }
                }
            }
        }
        if (budget < kGridHeader + 128u) budget = kGridHeader + 128u;         // room for every camera's grid at the coarsest block
        if (budget + 8 > s.grid.cap || !s.grid.ptr) {
            VC_TRY(ensure(ctx, s.grid, (size_t)budget + 8));                   // + padding: kernels copy it 16 bytes at a time
            VC_HIP(ctx, hipMemsetAsync(s.grid.ptr, 0, s.grid.cap * sizeof(uint32_t), st));
        }
        if (!s.boxes.ptr) {
            VC_TRY(ensure(ctx, s.boxes, (size_t)3 * kMaxCameras * kBoxStride));
            std::vector<uint32_t> init(s.boxes.cap, 0u);                       // both box sets start empty
            for (uint32_t k = 0; k < 2 * kMaxCameras; ++k) { init[kBoxStride * k] = 0xffffffffu; init[kBoxStride * k + 2] = 0xffffffffu; }
            VC_HIP(ctx, hipMemcpyAsync(s.boxes.ptr, init.data(), init.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            VC_HIP(ctx, hipStreamSynchronize(st));
            s.parity = 0;
        }
        s.budget_words = budget;
        s.parity ^= 1u;
        PrepParams pp;
        memset(&pp, 0, sizeof pp);
        for (uint32_t c = 0; c < C; ++c) {
            pp.src[c] = s.bytes.ptr + HW * c;
            if (!ctx->post_open[c] && !ctx->post_close[c]) continue;
            // MORPH_OPEN = erode, dilate; MORPH_CLOSE = dilate, erode (opening first when both are set); the uploaded
            // bytes stay as they are, the filtered image of camera c goes to d_morph[c]
            VC_TRY(ensure(ctx, ctx->d_morph, HW * (C + 1)));
            const uint8_t *img = s.bytes.ptr + HW * c;
            uint8_t *fin = ctx->d_morph.ptr + HW * c, *tmp = ctx->d_morph.ptr + HW * C;
            const dim3 mg(grid_for(HW)), mb(kBlock);
            if (ctx->post_open[c]) {
                hipLaunchKernelGGL((k_morph2x2<false>), mg, mb, 0, st, img, tmp, ctx->H, ctx->W);
                hipLaunchKernelGGL((k_morph2x2<true>), mg, mb, 0, st, (const uint8_t *)tmp, fin, ctx->H, ctx->W);
                img = fin;
            }
            if (ctx->post_close[c]) {
                hipLaunchKernelGGL((k_morph2x2<true>), mg, mb, 0, st, img, tmp, ctx->H, ctx->W);
                hipLaunchKernelGGL((k_morph2x2<false>), mg, mb, 0, st, (const uint8_t *)tmp, fin, ctx->H, ctx->W);
            }
            VC_HIP(ctx, hipGetLastError());
            pp.src[c] = fin;
        }
        for (uint32_t c = 0; c < C; ++c) {
            if (!s.frame_dirty[c]) continue;
            pp.fsrc[pp.nframes] = s.fbytes[c].ptr;
            pp.fdst[pp.nframes] = s.frames.ptr + HW * c;
            pp.nframes++;
            s.frame_dirty[c] = 0;
        }
        pp.bits = s.bits.ptr; pp.grid = s.grid.ptr; pp.boxes = s.boxes.ptr;
        pp.C = C; pp.H = ctx->H; pp.W = ctx->W; pp.HW = (uint32_t)HW; pp.mwords = ctx->mwords;
        pp.parity = s.parity;
        pp.dbg = (uint32_t)ctx->dbg;
        // about a thousand packing workgroups at most: every one of them looks at (and may update) its camera's box
        const uint64_t total_words = (uint64_t)ctx->mwords * C;
        pp.iters = (uint32_t)(total_words / (256ull * 1024ull));
        pp.iters = pp.iters < 1 ? 1 : (pp.iters > 16 ? 16 : pp.iters);
        const uint32_t pw = (ctx->mwords + kBlock * pp.iters - 1) / (kBlock * pp.iters), fw = (uint32_t)((HW + 4 * kBlock - 1) / (4 * kBlock));
        VC_KLAUNCH(VC_K_PREP_PACK, k_prep_pack, dim3(C * pw + pp.nframes * fw), dim3(kBlock), 0, st, pp);
        VC_HIP(ctx, hipGetLastError());
        s.bits_valid = true;
        s.grids_valid = false;
        s.counts_zero = true;
    }
    if (want_grids && !s.grids_valid) {
        CarveParams p = *cp;
        p.maskbits = s.bits.ptr;
        const uint64_t n = p.n;
        const uint32_t ns = (uint32_t)(n < kEstimateSamples ? n : kEstimateSamples);
        const uint32_t est_wgs = ctx->reorder ? (ns + kBlock * kEstPerThread - 1) / (kBlock * kEstPerThread) : 0u;   // no counts: cameras in index order
        if (!s.counts_zero) VC_HIP(ctx, hipMemsetAsync(s.boxes.ptr + kCountBase, 0, sizeof(uint32_t) * kMaxCameras * kBoxStride, st));
        s.counts_zero = false;
        // all grids together hold at most 16 blocks per budgeted word; every camera's blocks are rounded up to whole workgroups
        const uint32_t grid_wgs = (16u * s.budget_words + kBlock - 1) / kBlock + C;
        VC_KLAUNCH(VC_K_PREP_GRID, k_prep_grid, dim3(grid_wgs + est_wgs), dim3(kBlock), 0, st, p,
                           s.grid.ptr, s.boxes.ptr, s.parity, (uint32_t)ctx->grid_min_shift, s.budget_words, ns, grid_wgs);
        VC_HIP(ctx, hipGetLastError());
        // large grids (the brick pipeline's 1024-thread workgroups): the brick level gets 4 x 4 times coarser blocks
        s.has_coarse = false;
        if ((size_t)s.budget_words * sizeof(uint32_t) > kWideGridBytes) {
            VC_TRY(ensure(ctx, s.coarse, (size_t)s.budget_words + 8));       // (never larger than the fine grids)
            hipLaunchKernelGGL(k_coarsen_grids, dim3(8, C), dim3(kBlock), 0, st, (const uint32_t *)s.grid.ptr, s.coarse.ptr, C);
            VC_HIP(ctx, hipGetLastError());
            s.has_coarse = true;
        }
        s.grids_valid = true;
    }
    VC_HIP(ctx, hipEventRecord(s.e_prep, st));
    s.prep_pending = true;
    return VC_OK;
}

uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// vc_carve_footprint, on the carve stream in front of k_carve_foot: the grid's cell lattices (once per vc_set_grid) and the
// slot's summed-area tables (once per preparation of the slot; the caller has made the stream wait for that preparation).
// Lattice of an axis with n cells (include/voxcarve.h): h = 0.5 * ((hi - lo) / (n - 1)), 0 when n == 1; L[k] = c[k] - h, L[n] = c[n-1] + h
int ensure_footprint(vc_ctx *ctx, Slot &s)
{
    if (!ctx->foot_axes_valid) {
        const std::vector<double> *ax[3] = {&ctx->xs, &ctx->ys, &ctx->zs};
        std::vector<double> lat;
        for (int a = 0; a < 3; ++a) {
            const std::vector<double> &c = *ax[a];
            const size_t n = c.size();
            const double h = n > 1 ? 0.5 * ((ctx->bounds[2 * a + 1] - ctx->bounds[2 * a]) / (double)(n - 1)) : 0.0;
            for (size_t k = 0; k < n; ++k) lat.push_back(c[k] - h);
            lat.push_back(c[n - 1] + h);
        }
        VC_TRY(ensure(ctx, ctx->d_foot_axes, lat.size()));
        VC_HIP(ctx, hipMemcpy(ctx->d_foot_axes.ptr, lat.data(), lat.size() * sizeof(double), hipMemcpyHostToDevice));   // (pageable: synchronous)
        ctx->foot_axes_valid = true;
    }
    if (s.sat_valid && s.sat_gen == s.gen) return VC_OK;
    const uint32_t C = ctx->C, H = ctx->H, W = ctx->W;
    VC_TRY(ensure(ctx, s.sat, (size_t)C * (H + 1) * (W + 1)));
    hipEvent_t ks, ke;
    kev_pick(ctx, VC_K_FOOT_TABLE, ks, ke);                      // begin rides on the row pass, end on the column pass
    hipExtLaunchKernelGGL(k_foot_rows, dim3((C * H + 3) / 4), dim3(kBlock), 0, ctx->stream, ks, nullptr, 0, (const uint32_t *)s.bits.ptr,
                          s.sat.ptr, C, H, W, ctx->mwords);
    hipExtLaunchKernelGGL(k_foot_cols, dim3(grid_for((uint64_t)C * (W + 1))), dim3(kBlock), 0, ctx->stream, nullptr, ke, 0, s.sat.ptr, C, H, W);
    VC_HIP(ctx, hipGetLastError());
    s.sat_valid = true;
    s.sat_gen = s.gen;
    return VC_OK;
}

constexpr int kEmitBatch = 4;              // survivors per lane in flight together in k_emit_words

// The colour source of a step, one half of the expansion's parameters (everything else zero): axes and image size, and with a colour
// camera its model, its mask bits and its frame in the step's frame set.  For the step's own expansion and for vc_expand_entries'.
void emit_color_source(const vc_ctx *ctx, uint32_t slot, int color_cam, EmitParams &e)
{
    memset(&e, 0, sizeof e);
    e.xs = ctx->d_axes.ptr; e.ys = e.xs + ctx->nx; e.zs = e.ys + ctx->ny;
    e.nx = ctx->nx; e.ny = ctx->ny; e.H = ctx->H; e.W = ctx->W;
    if (color_cam < 0) return;
    const Slot &s = ctx->slots[slot];
    e.has_cam = 1;
    e.cam = ctx->cams[color_cam];
    e.maskbits = s.bits.ptr + (size_t)color_cam * ctx->mwords;
    if (s.frames.ptr && s.have_frame[color_cam]) e.frame = s.frames.ptr + (size_t)color_cam * ctx->H * ctx->W;
}

// start / stop: events that are to carry the launch's own begin and end (its packet's signals, hipExtLaunchKernelGGL), or null
int launch_emit(vc_ctx *ctx, StepBuf &sb, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr)
{
    const EmitParams &e = sb.emit;
    const dim3 eg((e.ngroups + 3) / 4), block(kBlock);
#define VC_EMIT(kernel, grid) hipExtLaunchKernelGGL((kernel), grid, block, 0, st, start, stop, 0, e)
    if (sb.route.busy && ctx->emit_lanes) {
        const dim3 bg(256u * (uint32_t)ctx->emit_waves_per_cu / 4u);
        if (e.lut16) VC_EMIT((k_emit_busy<true, true, 8, true>), bg);             // (ensure_lut16: steps that need every camera only)
        else if (e.lut && sb.route.allseen) VC_EMIT((k_emit_busy<true, true, 8>), bg);
        else if (e.lut) VC_EMIT((k_emit_busy<true, false, 8>), bg);
        else if (sb.route.allseen) VC_EMIT((k_emit_busy<false, true, 4>), bg);
        else VC_EMIT((k_emit_busy<false, false, 4>), bg);
    }
    else if (ctx->emit_lanes) {
        if (e.lut16) VC_EMIT((k_emit_lanes<true, true, 8, false, true>), eg);
        else if (e.lut && sb.route.allseen) VC_EMIT((k_emit_lanes<true, true, 8>), eg);
        else if (e.lut) VC_EMIT((k_emit_lanes<true, false, 8>), eg);
        else if (sb.route.allseen) VC_EMIT((k_emit_lanes<false, true, 4>), eg);
        else VC_EMIT((k_emit_lanes<false, false, 4>), eg);
    }
    else if (e.lut && sb.route.allseen) VC_EMIT((k_emit_words<true, true, kEmitBatch>), eg);
    else if (e.lut) VC_EMIT((k_emit_words<true, false, kEmitBatch>), eg);
    else if (sb.route.allseen) VC_EMIT((k_emit_words<false, true, kEmitBatch>), eg);
    else VC_EMIT((k_emit_words<false, false, kEmitBatch>), eg);
#undef VC_EMIT
    VC_HIP(ctx, hipGetLastError());
    ctx->last_emit16 = e.lut16 != nullptr && ctx->emit_lanes;
    return VC_OK;
}


// counts cnt (usually b.cnt) -> exclusive offsets b.off / b.boff (two levels) on stream st; the total also lands in *total_host and
// in b.boff[nscan]
int scan_counts(vc_ctx *ctx, hipStream_t st, ScanBufs &b, const uint32_t *cnt, uint32_t ngroups, uint64_t *total_host)
{
    const uint32_t nscan = (ngroups + kScanBlock - 1) / kScanBlock;
    hipLaunchKernelGGL(k_scan_groups, dim3(nscan), dim3(kScanThreads), 0, st, cnt, ngroups, b.off.ptr, b.bsum.ptr, b.boff.ptr, total_host,
                       (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u);
    VC_HIP(ctx, hipGetLastError());
    if (nscan > 1) {
        hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(kScanThreads), 0, st, b.bsum.ptr, nscan, b.boff.ptr, total_host);
        VC_HIP(ctx, hipGetLastError());
    }
    return VC_OK;
}

constexpr int kThinKind = VC_KERNEL_KINDS;   // dist_events: the launches of vc_hull_thin (vc_timing_t::thin_kernel_ms, no vc_kernel_kind)

// timing_detail: the begin / end events a launch of the distance passes is to carry (null otherwise: an ordinary launch)
static void dist_events(vc_ctx *ctx, int kind, hipEvent_t &start, hipEvent_t &stop)
{
    start = stop = nullptr;
    if (!ctx->timing_detail) return;
    const size_t at = 2 * ctx->dist_ev_kind.size();
    while (ctx->dist_ev.size() < at + 2) {
        Event e;
        if (make_event(e) != hipSuccess) return;
        ctx->dist_ev.push_back(std::move(e));
    }
    start = ctx->dist_ev[at]; stop = ctx->dist_ev[at + 1];
    ctx->dist_ev_kind.push_back(kind);
}
#define VC_DLAUNCH(kind, kernel, grid, block, ...)                                                      \
    do {                                                                                                \
        hipEvent_t ks_, ke_;                                                                            \
        dist_events(ctx, kind, ks_, ke_);                                                               \
        hipExtLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, ks_, ke_, 0, __VA_ARGS__);           \
    } while (0)

// Survivors before each occupancy word of the step, as vc_components.h counts them, into woff[nwords]: popcounts per 64 words,
// their scan in ctx->d_rscan, the wave scan inside each group.  The survivor total lands in *total_host once the stream has
// drained.  kind >= 0: the launches carry that kind's events (VC_DLAUNCH).  Buffers sized by the caller (d_rscan: word_groups).
static uint32_t word_groups(uint64_t nwords) { return (uint32_t)((nwords + 63) / 64); }   // 64 words per group: <= 2^20 groups

static int word_offsets(vc_ctx *ctx, const StepBuf &cur, uint64_t nwords, DevBuf<uint32_t> &woff, uint64_t *total_host, int kind = -1)
{
    const uint32_t wgroups = word_groups(nwords);
    const dim3 wgrid((wgroups + kCcBlock / 64 - 1) / (kCcBlock / 64)), block(kCcBlock);
    const uint64_t *words = cur.words.ptr;
    if (kind >= 0) VC_DLAUNCH(kind, k_cc_wcount, wgrid, block, words, nwords, wgroups, ctx->d_rscan.cnt.ptr);
    else hipLaunchKernelGGL(k_cc_wcount, wgrid, block, 0, ctx->stream, words, nwords, wgroups, ctx->d_rscan.cnt.ptr);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_rscan, ctx->d_rscan.cnt.ptr, wgroups, total_host));
    const uint32_t *off = ctx->d_rscan.off.ptr;                  // (read-only to k_cc_woff, as the words are)
    const uint64_t *boff = ctx->d_rscan.boff.ptr;
    if (kind >= 0) VC_DLAUNCH(kind, k_cc_woff, wgrid, block, words, nwords, wgroups, off, boff, woff.ptr);
    else hipLaunchKernelGGL(k_cc_woff, wgrid, block, 0, ctx->stream, words, nwords, wgroups, off, boff, woff.ptr);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// Stable compaction of records [0, S) by sel (vc_compact.h) on the context's stream, in the scan scratch of the passes over the
// result (ctx->d_rscan); the count lands in *total_host once the stream has drained, and in d_rscan.boff[nscan].
template <class Sel>
int compact(vc_ctx *ctx, const Sel &sel, uint64_t S, uint64_t *total_host)
{
    const uint32_t ngroups = (uint32_t)((S + kCompactGroup - 1) / kCompactGroup);
    VC_TRY(ensure(ctx, ctx->d_rscan, ngroups));
    hipLaunchKernelGGL(k_compact_count<Sel>, dim3(ngroups), dim3(kCompactBlock), 0, ctx->stream, S, ctx->d_rscan.cnt.ptr, sel);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_rscan, ctx->d_rscan.cnt.ptr, ngroups, total_host));
    hipLaunchKernelGGL(k_compact_scatter<Sel>, dim3(ngroups), dim3(kCompactBlock), 0, ctx->stream, S,
                       (const uint32_t *)ctx->d_rscan.off.ptr, (const uint64_t *)ctx->d_rscan.boff.ptr, sel);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// The spare buffer holds the new records of the current result, d_rscan the scan (over ngroups groups) whose total is their number:
// the buffers are swapped, and the readers of the step's scan (vc_pack_entries / the compact gather report blockoff[nscan] as
// this rank's survivors) get that total.
int records_handed_over(vc_ctx *ctx, StepBuf &cur, uint32_t ngroups)
{
    std::swap(cur.records, ctx->d_rec_spare);
    const uint32_t nscan = (ngroups + kScanBlock - 1) / kScanBlock;
    const uint64_t n_pad = (cur.n + kLutPad - 1) / kLutPad * kLutPad;
    const uint32_t cscan = (uint32_t)((n_pad / (64 * kGroupWords) + kScanBlock - 1) / kScanBlock);
    VC_HIP(ctx, hipMemcpyAsync(cur.blockoff.ptr + cscan, ctx->d_rscan.boff.ptr + nscan, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                               ctx->stream));
    cur.nz_valid = false;                        // non-zero word counts per group: counted again by the next packing
    ctx->gathered = false; ctx->packed = false;
    return VC_OK;
}

// The records of the current result that sel keeps (sel.out: the copy's target) become the result, in record order: compacted
// into the spare buffer, which is then swapped with the step's.  The caller sets the survivors to the count, which lands in
// *total_host once the stream has drained.
template <class Sel>
int compact_records(vc_ctx *ctx, StepBuf &cur, Sel sel, uint64_t S, uint64_t *total_host)
{
    VC_TRY(ensure(ctx, ctx->d_rec_spare, cur.records.cap));
    sel.out = ctx->d_rec_spare.ptr;
    VC_TRY(compact(ctx, sel, S, total_host));
    return records_handed_over(ctx, cur, (uint32_t)((S + kCompactGroup - 1) / kCompactGroup));
}

// ---- the other route to new records: the occupancy gained (and possibly lost) voxels (vc_merge.h) ----
// A pass of this kind (vc_hull_grow, vc_hull_temporal) marks or votes and reads the new count S1 back; then merge_sized, its change
// of the words, merge_ranked, its own kernel over the words for the fresh records, records_handed_over; after pass_end, merge_counted.
int merge_refuse_slot(vc_ctx *ctx, const char *what, const StepBuf &cur)
{
    if (cur.slot < ctx->slots.size() && ctx->slots[cur.slot].gen == cur.slot_gen) return VC_OK;
    return fail(ctx, VC_ERR_ARG, "%s: frame set %u has been prepared again since the carve: its images are not the ones "
                "the records' colours came from", what, cur.slot);
}

int merge_refuse_index(vc_ctx *ctx, const char *what, uint64_t n)
{
    return n > 0xffffffffull ? fail(ctx, VC_ERR_ARG, "%s: %llu voxels exceed the u32 index", what, (unsigned long long)n) : VC_OK;
}

// Every buffer of the route, before result, ring or P is touched (a failed allocation leaves them all as they were), and the kernels'
// parameters, which point into them.  records = false: only the ranks are wanted; added: the pass's own [S1] bytes, zeroed
int merge_sized(vc_ctx *ctx, const StepBuf &cur, uint64_t nwords, uint64_t S1, bool records, uint8_t *added, MergeParams &p)
{
    VC_TRY(ensure(ctx, ctx->d_rscan, word_groups(nwords)));
    VC_TRY(ensure(ctx, ctx->d_woff, (size_t)nwords));
    if (records) VC_TRY(ensure(ctx, ctx->d_rec_spare, std::max<size_t>(cur.records.cap, (size_t)S1)));
    memset(&p, 0, sizeof p);
    p.xs = cur.emit.xs; p.ys = cur.emit.ys; p.zs = cur.emit.zs;
    p.has_cam = cur.emit.has_cam && cur.emit.xs ? 1 : 0;
    p.cam = cur.emit.cam;
    p.frame = cur.emit.frame;
    p.words = cur.words.ptr; p.woff = ctx->d_woff.ptr;
    p.out = ctx->d_rec_spare.ptr; p.added = added;
    p.S1 = S1;
    p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz; p.H = ctx->H; p.W = ctx->W;
    return VC_OK;
}

// Ranks of the occupancy into d_woff, their total into h_res[2].  changed: the words are new, so the survivors per group of the step
// are counted again (the packing skips the groups whose count is zero) and every old record that stays goes to its new rank in the
// spare buffer.  The launches run under the pass's two kinds (a kind of -1: they carry none, as word_offsets').
int merge_ranked(vc_ctx *ctx, StepBuf &cur, const MergeParams &p, uint64_t nwords, uint64_t S0, bool changed, int rank_kind, int merge_kind)
{
    if (changed) {
        const uint32_t sgroups = (uint32_t)((cur.n + kLutPad - 1) / kLutPad * kLutPad / (64 * kGroupWords));
        const dim3 cgrid((sgroups + 3) / 4), cblock(kBlock);
        if (rank_kind >= 0) VC_DLAUNCH(rank_kind, k_count_groups, cgrid, cblock, (const uint64_t *)cur.words.ptr, nwords, sgroups, cur.groupcnt.ptr);
        else hipLaunchKernelGGL(k_count_groups, cgrid, cblock, 0, ctx->stream, (const uint64_t *)cur.words.ptr, nwords, sgroups, cur.groupcnt.ptr);
    }
    VC_TRY(word_offsets(ctx, cur, nwords, ctx->d_woff, ctx->h_res + 2, rank_kind));
    const dim3 ogrid((uint32_t)((S0 + kMergeBlock - 1) / kMergeBlock)), oblock(kMergeBlock);
    if (changed && S0) {
        if (merge_kind >= 0) VC_DLAUNCH(merge_kind, k_merge_old, ogrid, oblock, p, (const uint64_t *)cur.records.ptr, S0, nwords);
        else hipLaunchKernelGGL(k_merge_old, ogrid, oblock, 0, ctx->stream, p, (const uint64_t *)cur.records.ptr, S0, nwords);
    }
    return VC_OK;
}

// after pass_end; `how` ends the pass's own message
int merge_counted(vc_ctx *ctx, const char *what, uint64_t S1, const char *how)
{
    if (ctx->h_res[2] == S1) return VC_OK;
    return fail(ctx, VC_ERR_HIP, "%s: the new occupancy holds %llu voxels, %llu %s", what, (unsigned long long)ctx->h_res[2], (unsigned long long)S1, how);
}

int ensure_exchange_scratch(vc_ctx *ctx, uint32_t ngroups)
{
    VC_TRY(ensure(ctx, ctx->d_xscan, ngroups));
    VC_HIP(ctx, ensure_pinned(ctx->h_xtotal, 4));                // [2], [3]: the two gathers in flight
    return VC_OK;
}

// Pixel boxes of the slab's words (tile or y-line order) without a lookup table: the table-free
// hierarchical kernel reads them instead of bounding each word by interval arithmetic.  Geometry only:
// built once per grid / slab / camera set (the projection of every voxel, as long as vc_build_lut).
int ensure_boxes(vc_ctx *ctx, bool tile)
{
    if (tile ? ctx->tbox_valid : ctx->bbox_valid) return VC_OK;
    const uint64_t n = ctx->n_voxels();
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    DevBuf<uint64_t> &buf = tile ? ctx->d_tbox : ctx->d_bbox;
    VC_TRY(ensure(ctx, buf, (size_t)(n_pad / 64) * ctx->C));
    CarveParams p;
    fill_params(ctx, p);
    if (tile) hipLaunchKernelGGL(k_build_lut<true>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, (int32_t *)nullptr, buf.ptr);
    else hipLaunchKernelGGL(k_build_lut<false>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, (int32_t *)nullptr, buf.ptr);
    VC_HIP(ctx, hipGetLastError());
    (tile ? ctx->tbox_valid : ctx->bbox_valid) = true;
    if (tile) VC_TRY(build_brick_boxes(ctx));
    return VC_OK;
}

// Enqueues the packing of the current result's non-zero words into ctx->d_ent ({bits, base} pairs) and
// {entries, survivors} into ctx->d_mine.  No host synchronisation; *h_xtotal holds the entry count
// once the stream has drained.
int enqueue_pack(vc_ctx *ctx, StepBuf &cur, hipStream_t st)
{
    const uint64_t n = cur.n;
    VC_TRY(ensure_exchange_scratch(ctx, 1));
    VC_TRY(ensure(ctx, cur.mine, 2));
    if (n == 0) {
        VC_HIP(ctx, hipMemsetAsync(cur.mine.ptr, 0, 2 * sizeof(uint64_t), st));
        *ctx->h_xtotal = 0;
        return VC_OK;
    }
    const uint64_t nwords = (n + 63) / 64;
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    const uint32_t ngroups = (uint32_t)(n_pad / (64 * kGroupWords));
    const uint32_t nscan = (ngroups + kScanBlock - 1) / kScanBlock;
    VC_TRY(ensure_exchange_scratch(ctx, ngroups));
    VC_TRY(ensure(ctx, cur.ent, (size_t)(2 * nwords)));          // worst case: every word non-zero (n / 4 bytes)
    const dim3 grid((ngroups + 3) / 4), block(kBlock);
    if (cur.nz_valid && cur.route.busy) {
        // the carve left the counts of non-zero words and the list of groups with survivors: no counting pass, and the packing
        // strides over the list (5 of 6 groups are empty; a launch over all of them is dispatch bound)
        VC_TRY(scan_counts(ctx, st, ctx->d_xscan, cur.groupnz.ptr, ngroups, ctx->h_xtotal));
        hipLaunchKernelGGL(k_pack_busy, dim3(1024), block, 0, st, (const uint64_t *)cur.words.ptr, nwords, (const uint32_t *)cur.busylist.ptr,
                           (const uint32_t *)cur.busyblock.ptr, (const uint32_t *)ctx->d_xscan.off.ptr, (const uint64_t *)ctx->d_xscan.boff.ptr, nscan, ctx->i0(),
                           (const uint64_t *)(cur.blockoff.ptr + nscan), cur.ent.ptr, cur.mine.ptr);
        VC_HIP(ctx, hipGetLastError());
        return VC_OK;
    }
    hipLaunchKernelGGL(k_count_nz, grid, block, 0, st, cur.words.ptr, nwords, ngroups, cur.groupcnt.ptr,
                       ctx->d_xscan.cnt.ptr);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(scan_counts(ctx, st, ctx->d_xscan, ctx->d_xscan.cnt.ptr, ngroups, ctx->h_xtotal));
    hipLaunchKernelGGL(k_pack_entries, grid, block, 0, st, cur.words.ptr, nwords, ngroups, cur.groupcnt.ptr, ctx->d_xscan.off.ptr,
                       ctx->d_xscan.boff.ptr, nscan, ctx->i0(), cur.blockoff.ptr + nscan, cur.ent.ptr, cur.mine.ptr);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// {entries, survivors} of every rank into cur.h_counts (valid once the stream has drained).
int enqueue_counts_exchange(vc_ctx *ctx, StepBuf &cur, hipStream_t st)
{
    const int G = ctx->n_ranks;
    VC_TRY(ensure(ctx, cur.counts, (size_t)2 * G));
    VC_HIP(ctx, ensure_pinned(cur.h_counts, 2 * VC_MAX_RANKS));
    VC_NCCL(ctx, g_rccl.AllGather(cur.mine.ptr, cur.counts.ptr, 2, ncclUint64, ctx->comm, st));
    VC_HIP(ctx, hipMemcpyAsync(cur.h_counts, cur.counts.ptr, sizeof(uint64_t) * 2 * G, hipMemcpyDeviceToHost, st));
    return VC_OK;
}

// The colour camera's table over the whole grid (4 B per voxel of the WHOLE grid, built once per
// camera): what lets a rank colour survivors of words another rank carved.
int ensure_color_table(vc_ctx *ctx, int cam)
{
    if (ctx->lut_color_cam == cam && ctx->d_lut_color.ptr) return VC_OK;
    // another camera's table goes into the same buffer: the expansion of a step still in flight (or of a queued gather) may be
    // reading the old one on its own stream.  The projection waits for it on the device; the host does not.
    if (ctx->lut_color_reader) {
        VC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->lut_color_reader, 0));
        ctx->lut_color_reader = nullptr;
    }
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    VC_TRY(ensure(ctx, ctx->d_lut_color, (size_t)n_pad));
    CarveParams p;
    fill_params(ctx, p);
    p.n = n; p.n_pad = n_pad; p.z0 = 0; p.C = 1;
    p.cam[0] = ctx->cams[cam];
    hipLaunchKernelGGL(k_build_lut<false>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, ctx->d_lut_color.ptr,
                       (uint64_t *)nullptr);
    VC_HIP(ctx, hipGetLastError());
    ctx->lut_color_cam = cam;
    return VC_OK;
}

// The colour camera's compact table for the expansion of VC_MODE_LUT (see vc_ctx::d_lut16), packed from d_lut_tile on the
// carve stream by the first step that names the camera -- in front of the step's carve kernels, like the table above, so
// that {scan done} orders the expansion stream behind it.  use = the step may read it: the camera's table fits 16 bits per
// entry.  The verdict is read back once, here (first use: the streams drain); a camera that does not fit, or a device without
// the memory, keeps the 4-byte entries and is not tried again until the table changes.
int ensure_lut16(vc_ctx *ctx, int cam, uint64_t n_pad, bool &use)
{
    use = false;
    if ((ctx->lut16_nofit >> cam) & 1u) return VC_OK;
    if (ctx->lut16_cam == cam) { use = true; return VC_OK; }
    // (an expansion in flight may still read the table of the camera before)
    if (ctx->lut16_cam >= 0 && ctx->npending) VC_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    ctx->lut16_cam = -1;
    VC_TRY(ensure(ctx, ctx->d_lut16_flag, 1));
    auto room = [](auto &b, size_t elems) {
        if (b.ptr && b.cap >= elems) return true;
        b.reset();
        if (hipMalloc(reinterpret_cast<void **>(&b.ptr), elems * sizeof(*b.ptr)) != hipSuccess) { (void)hipGetLastError(); b.ptr = nullptr; return false; }
        b.cap = elems;
        return true;
    };
    if (!room(ctx->d_lut16, (size_t)n_pad) || !room(ctx->d_cbase, (size_t)(n_pad / 64))) {
        ctx->d_lut16.reset(); ctx->d_cbase.reset();
        ctx->lut16_nofit |= 1u << cam;
        return VC_OK;
    }
    VC_HIP(ctx, hipMemsetAsync(ctx->d_lut16_flag.ptr, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_pack_lut16, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, (const int32_t *)(ctx->d_lut_tile.ptr + (size_t)cam * n_pad),
                       ctx->d_lut16.ptr, ctx->d_cbase.ptr, ctx->d_lut16_flag.ptr);
    VC_HIP(ctx, hipGetLastError());
    uint32_t nofit = 0;
    VC_HIP(ctx, hipMemcpyAsync(&nofit, ctx->d_lut16_flag.ptr, sizeof nofit, hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (nofit) { ctx->lut16_nofit |= 1u << cam; return VC_OK; }
    ctx->lut16_cam = cam;
    use = true;
    return VC_OK;
}

// Observes the completion of a queued all-gather: its timing, and that the expansion produced
// the survivor count the ranks announced.
static int finish_one(vc_ctx *ctx, uint32_t half)
{
    if (!ctx->gpend[half]) return VC_OK;
    ctx->gpend[half] = false;
    Event *E = ctx->gx[ctx->gx_idx[half]];
    VC_HIP(ctx, hipEventSynchronize(E[1]));
    VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.gather_ms, E[0], E[1]));
    VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.exchange_ms, E[0], E[2]));
    ctx->tm.gather_ms_sum += ctx->tm.gather_ms;
    ctx->tm.gathers += 1;
    if (ctx->gexpect[half] && ctx->h_xtotal[2 + half] != ctx->gexpect[half])
        return fail(ctx, VC_ERR_RCCL, "gathered words expand to %llu survivors, the ranks reported %llu",
                    (unsigned long long)ctx->h_xtotal[2 + half], (unsigned long long)ctx->gexpect[half]);
    return VC_OK;
}
// every queued compact gather, oldest first
int finish_gather(vc_ctx *ctx)
{
    VC_TRY(finish_one(ctx, ctx->gseq & 1u));
    return finish_one(ctx, (ctx->gseq + 1u) & 1u);
}

// Expands M gathered entries (device, ascending) into the ordered survivor records of the whole grid
// in ctx->d_gathered, coloured the way the current step was (its mode, colour camera and frame set).
// S_hint = expected survivor count (0 = unknown: sized after a host synchronisation).
// st: the stream the expansion runs on (the second stream lets it run beside the next step's carve; its scan
// scratch is its own because the next step's packing may be under way on the first).
int enqueue_expand(vc_ctx *ctx, hipStream_t st, const uint64_t *d_entries, uint64_t M, uint64_t S_hint, uint64_t *h_total = nullptr)
{
    StepBuf &cur = ctx->sb[ctx->cur];
    if (!h_total) h_total = ctx->h_xtotal + 1;                   // (page-locked word the scan leaves the survivor total in)
    *h_total = 0;
    if (M == 0) return VC_OK;
    const uint32_t chunk = M <= (1ull << 24) ? 16u : kGroupWords;   // entries per wave (the scan takes 2^20 groups at most)
    const uint32_t ngroups = (uint32_t)((M + chunk - 1) / chunk);
    VC_TRY(ensure_exchange_scratch(ctx, 1));
    VC_TRY(ensure(ctx, ctx->d_yscan, ngroups));
    // (the table-free mode colours from the colour camera's table too, unless fused_color_table is off: the whole-grid table the
    // expansion of other ranks' words needs is the very one)
    const bool from_lut = (cur.route.lut || ctx->fused_color_table) && cur.color_cam >= 0;
    if (from_lut && !(ctx->lut_color_cam == cur.color_cam && ctx->d_lut_color.ptr)) {
        VC_TRY(ensure_color_table(ctx, cur.color_cam));           // built on the first stream, once per camera
        if (st != ctx->stream) VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const dim3 grid((ngroups + 3) / 4), block(kBlock);
    hipLaunchKernelGGL(k_count_entries, chunk == 16u ? dim3((ngroups + 15) / 16) : grid, block, 0, st, d_entries, M, ngroups, ctx->d_yscan.cnt.ptr, chunk);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(scan_counts(ctx, st, ctx->d_yscan, ctx->d_yscan.cnt.ptr, ngroups, h_total));
    if (S_hint == 0) {
        VC_HIP(ctx, hipStreamSynchronize(st));
        S_hint = *h_total;
    }
    if (S_hint > ctx->d_gathered.cap)            // survivor counts drift from frame to frame: grow with slack
        VC_TRY(ensure(ctx, ctx->d_gathered, (size_t)(S_hint + S_hint / 8 + 1024)));
    EmitParams e;
    emit_color_source(ctx, cur.slot, cur.color_cam, e);          // axes, camera, mask bits and frame of the step
    e.entries = d_entries;
    e.groupcnt = ctx->d_yscan.cnt.ptr; e.groupoff = ctx->d_yscan.off.ptr; e.blockoff = ctx->d_yscan.boff.ptr;
    e.n = M * 64; e.i0 = 0; e.z0 = 0; e.ngroups = ngroups; e.entry_chunk = chunk;
    e.records = ctx->d_gathered.ptr; e.capacity = ctx->d_gathered.cap;
    e.lut = from_lut ? ctx->d_lut_color.ptr : nullptr;
    if (from_lut && cur.route.allseen) hipLaunchKernelGGL((k_emit_lanes<true, true, 8, true>), grid, block, 0, st, e);
    else if (from_lut) hipLaunchKernelGGL((k_emit_lanes<true, false, 8, true>), grid, block, 0, st, e);
    else if (cur.route.allseen) hipLaunchKernelGGL((k_emit_lanes<false, true, 4, true>), grid, block, 0, st, e);
    else hipLaunchKernelGGL((k_emit_lanes<false, false, 4, true>), grid, block, 0, st, e);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

}  // namespace

// ================================================================ C ABI
// (every entry point is declared extern "C" by include/voxcarve.h: its definition takes that linkage; helpers are static)
int vc_device_count(int *n_out)
{
    if (!n_out) return VC_ERR_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *n_out = 0; return fail(nullptr, VC_ERR_NODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n_out = n;
    return VC_OK;
}

int vc_create(int device, vc_ctx **out)
{
    if (!out) return VC_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, VC_ERR_NODEV, "no HIP device (%s); voxcarve has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "count 0");
    if (device < 0 || device >= n) return fail(nullptr, VC_ERR_ARG, "device %d not in [0,%d)", device, n);
    hipDeviceProp_t prop;
    VC_HIP(nullptr, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, VC_ERR_NODEV, "device %d is %s; this library carries gfx950 code only",
                    device, prop.gcnArchName);
    VC_HIP(nullptr, hipSetDevice(device));
    vc_ctx *ctx = new vc_ctx();
    ctx->device = device;
    memset(&ctx->tm, 0, sizeof ctx->tm);
    hipError_t e1 = make_streams(ctx);
    for (int k = 0; k < 2 && e1 == hipSuccess; ++k) e1 = make_event(ctx->ev_h[k]);
    for (int k = 0; k < kDepth && e1 == hipSuccess; ++k) {
        StepBuf &b = ctx->sb[k];
        for (Event *ev : {&b.e0, &b.e_first, &b.e1, &b.e_prep})
            if (e1 == hipSuccess) e1 = make_event(*ev);
        if (e1 == hipSuccess) e1 = ensure_pinned(b.h_total, 1);
    }
    for (int i = 0; i < 4 && e1 == hipSuccess; ++i) e1 = make_event(ctx->ev[i]);
    for (uint32_t r = 0; r < kGatherRing && e1 == hipSuccess; ++r)
        for (int i = 0; i < 3 && e1 == hipSuccess; ++i) e1 = make_event(ctx->gx[r][i]);
    if (e1 == hipSuccess) e1 = make_events(ctx);
    if (e1 == hipSuccess) e1 = ensure_pinned(ctx->h_total, 1);
    const char *fg = getenv("VOXCARVE_FORCE_GENERIC");
    ctx->force_generic = fg && fg[0] == '1';
    if (e1 != hipSuccess) {
        int rc = fail(nullptr, VC_ERR_HIP, "context setup: %s", hipGetErrorString(e1));
        vc_destroy(ctx);                 // releases whatever was created so far
        return rc;
    }
    *out = ctx;
    return VC_OK;
}

int vc_destroy(vc_ctx *ctx)
{
    if (!ctx) return VC_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t streams[4] = {ctx->stream2, ctx->stream_up, ctx->stream_x, ctx->stream};
    for (hipStream_t st : streams) if (st) (void)hipStreamSynchronize(st);
    if (ctx->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(ctx->comm);
    // every stream has drained: the context's members free their buffers, page-locked memory and events; the streams go last
    delete ctx;
    for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
    return VC_OK;
}

const char *vc_last_error(const vc_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int vc_synchronize(vc_ctx *ctx)
{
    if (!ctx) return VC_ERR_ARG;
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_x));
    return finish_gather(ctx);
}

int vc_set_grid(vc_ctx *ctx, uint32_t nx, uint32_t ny, uint32_t nz, const double bounds[6])
{
    if (!ctx || !bounds) return VC_ERR_ARG;
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (nx == 0 || ny == 0 || nz == 0) return fail(ctx, VC_ERR_ARG, "grid dimensions must be >= 1");
    const uint64_t N = (uint64_t)nx * ny * nz;
    if (N > 0xffffffffull || (uint64_t)nx * ny > 0xffffffffull)
        return fail(ctx, VC_ERR_ARG, "grid of %llu voxels exceeds the u32 voxel index", (unsigned long long)N);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->nx = nx; ctx->ny = ny; ctx->nz = nz; ctx->z0 = 0; ctx->z1 = nz;
    memcpy(ctx->bounds, bounds, sizeof ctx->bounds);
    linspace(bounds[0], bounds[1], nx, ctx->xs);
    linspace(bounds[2], bounds[3], ny, ctx->ys);
    linspace(bounds[4], bounds[5], nz, ctx->zs);
    VC_TRY(ensure(ctx, ctx->d_axes, (size_t)nx + ny + nz));
    VC_HIP(ctx, hipMemcpyAsync(ctx->d_axes.ptr, ctx->xs.data(), sizeof(double) * nx, hipMemcpyHostToDevice, ctx->stream));
    VC_HIP(ctx, hipMemcpyAsync(ctx->d_axes.ptr + nx, ctx->ys.data(), sizeof(double) * ny, hipMemcpyHostToDevice, ctx->stream));
    VC_HIP(ctx, hipMemcpyAsync(ctx->d_axes.ptr + nx + ny, ctx->zs.data(), sizeof(double) * nz, hipMemcpyHostToDevice, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_grid = true;
    ctx->foot_axes_valid = false;
    for (Slot &sl : ctx->slots) sl.grids_valid = false;       // the camera order was sampled on the old geometry
    if (ctx->h_lists) ctx->h_lists[0] = ctx->h_lists[1] = ctx->h_lists[2] = 0xffffffffu;
    geometry_changed(ctx);
    ctx->lut_color_cam = -1; ctx->packed = false;
    return VC_OK;
}

int vc_set_slab(vc_ctx *ctx, uint32_t z0, uint32_t z1)
{
    if (!ctx) return VC_ERR_ARG;
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->have_grid) return fail(ctx, VC_ERR_ARG, "vc_set_grid must precede vc_set_slab");
    if (z0 > z1 || z1 > ctx->nz) return fail(ctx, VC_ERR_ARG, "slab [%u,%u) outside [0,%u]", z0, z1, ctx->nz);
    ctx->z0 = z0; ctx->z1 = z1;
    for (Slot &sl : ctx->slots) sl.grids_valid = false;
    geometry_changed(ctx);
    ctx->packed = false;
    return VC_OK;
}

int vc_get_axes(vc_ctx *ctx, double *xs, double *ys, double *zs)
{
    if (!ctx || !ctx->have_grid) return ctx ? fail(ctx, VC_ERR_ARG, "no grid") : VC_ERR_ARG;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (xs) VC_HIP(ctx, hipMemcpy(xs, ctx->d_axes.ptr, sizeof(double) * ctx->nx, hipMemcpyDeviceToHost));
    if (ys) VC_HIP(ctx, hipMemcpy(ys, ctx->d_axes.ptr + ctx->nx, sizeof(double) * ctx->ny, hipMemcpyDeviceToHost));
    if (zs) VC_HIP(ctx, hipMemcpy(zs, ctx->d_axes.ptr + ctx->nx + ctx->ny, sizeof(double) * ctx->nz, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_set_cameras(vc_ctx *ctx, uint32_t C, const double *K9, const double *dist5, const double *R9,
                   const double *t3, uint32_t H, uint32_t W)
{
    if (!ctx || !K9 || !dist5 || !R9 || !t3) return VC_ERR_ARG;
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (C == 0 || C > VC_MAX_CAMERAS) return fail(ctx, VC_ERR_ARG, "camera count %u not in [1,%d]", C, VC_MAX_CAMERAS);
    if (H == 0 || W == 0 || H > 32767 || W > 65535) return fail(ctx, VC_ERR_ARG, "mask size %ux%u outside 1..32767 x 1..65535", H, W);
    for (uint32_t c = 0; c < C; ++c) {
        CamDev &d = ctx->cams[c];
        memcpy(d.r, R9 + 9 * c, sizeof d.r);
        memcpy(d.t, t3 + 3 * c, sizeof d.t);
        d.fx = K9[9 * c + 0]; d.cx = K9[9 * c + 2];
        d.fy = K9[9 * c + 4]; d.cy = K9[9 * c + 5];
        d.k1 = dist5[5 * c + 0]; d.k2 = dist5[5 * c + 1];
        d.p1 = dist5[5 * c + 2]; d.p2 = dist5[5 * c + 3];
        d.k3 = dist5[5 * c + 4];
    }
    const bool reshaped = (C != ctx->C || H != ctx->H || W != ctx->W);
    ctx->C = C; ctx->H = H; ctx->W = W;
    ctx->mwords = (uint32_t)(((uint64_t)H * W + 31) / 32);
    ctx->have_cams = true;
    (void)hipSetDevice(ctx->device);
    if (reshaped) {
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream2));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
        for (Slot &s : ctx->slots) release_slot(s);
    }
    for (Slot &sl : ctx->slots) sl.grids_valid = false;
    geometry_changed(ctx);
    ctx->lut_color_cam = -1; ctx->packed = false;
    return VC_OK;
}

// Host -> device copy of `bytes` into dst through the page-locked buffer *h_stage (grown on demand), on the upload
// stream.  The host only ever waits for ITS OWN previous copy out of that staging buffer; the copy itself waits (on
// the device) for the kernels that still read the bytes it replaces.
static int stage_upload(vc_ctx *ctx, Slot &s, Pinned<uint8_t> &h_stage, uint8_t *dst, const uint8_t *src, size_t bytes, bool timed)
{
    if (s.up_pending) { VC_HIP(ctx, hipEventSynchronize(s.e_up)); s.up_pending = false; }
    VC_HIP(ctx, ensure_pinned(h_stage, bytes));
    memcpy(h_stage, src, bytes);
    if (timed) {
        if (ctx->h2d_pending) { (void)hipEventSynchronize(ctx->ev_h[1]); (void)hipEventElapsedTime(&ctx->tm.h2d_ms, ctx->ev_h[0], ctx->ev_h[1]); }
        VC_HIP(ctx, hipEventRecord(ctx->ev_h[0], ctx->stream_up));
    }
    VC_HIP(ctx, hipMemcpyAsync(dst, h_stage, bytes, hipMemcpyHostToDevice, ctx->stream_up));
    if (timed) { VC_HIP(ctx, hipEventRecord(ctx->ev_h[1], ctx->stream_up)); ctx->h2d_pending = true; }
    VC_HIP(ctx, hipEventRecord(s.e_up, ctx->stream_up));
    s.up_pending = true;
    return VC_OK;
}

int vc_upload_masks(vc_ctx *ctx, uint32_t slot, const uint8_t *masks)
{
    if (!ctx || !masks) return VC_ERR_ARG;
    Slot *s = nullptr;
    VC_TRY(slot_at(ctx, slot, &s));
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)ctx->H * ctx->W;
    VC_TRY(ensure(ctx, s->bytes, HW * ctx->C + 64));
    VC_TRY(stage_upload(ctx, *s, s->h_bytes, s->bytes.ptr, masks, HW * ctx->C, true));
    s->have_masks = true;
    s->bits_valid = false;           // the next carve on this slot re-derives bits, grids and camera order on the device
    s->grids_valid = false;
    return VC_OK;
}

int vc_touch_masks(vc_ctx *ctx, uint32_t slot)
{
    if (!ctx) return VC_ERR_ARG;
    if (slot >= ctx->slots.size() || !ctx->slots[slot].have_masks) return fail(ctx, VC_ERR_ARG, "no masks uploaded in slot %u", slot);
    Slot &s = ctx->slots[slot];
    s.bits_valid = false;
    s.grids_valid = false;
    for (uint32_t c = 0; c < ctx->C; ++c) if (s.have_frame[c]) s.frame_dirty[c] = 1;
    return VC_OK;
}

int vc_set_mask_postfilter(vc_ctx *ctx, const uint8_t *open2x2, const uint8_t *close2x2)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->have_cams) return fail(ctx, VC_ERR_ARG, "vc_set_cameras must precede vc_set_mask_postfilter");
    for (uint32_t c = 0; c < VC_MAX_CAMERAS; ++c) {
        ctx->post_open[c] = (open2x2 && c < ctx->C) ? (open2x2[c] != 0) : 0;
        ctx->post_close[c] = (close2x2 && c < ctx->C) ? (close2x2[c] != 0) : 0;
    }
    return VC_OK;
}

int vc_fetch_mask(vc_ctx *ctx, uint32_t slot, uint32_t cam, uint8_t *out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    if (slot >= ctx->slots.size() || !ctx->slots[slot].have_masks) return fail(ctx, VC_ERR_ARG, "no masks uploaded in slot %u", slot);
    if (cam >= ctx->C) return fail(ctx, VC_ERR_ARG, "camera %u not in [0,%u)", cam, ctx->C);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(ensure_prepared(ctx, ctx->slots[slot], false, nullptr));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
    std::vector<uint32_t> bits(ctx->mwords);
    VC_HIP(ctx, hipMemcpy(bits.data(), ctx->slots[slot].bits.ptr + (size_t)cam * ctx->mwords, sizeof(uint32_t) * ctx->mwords,
                          hipMemcpyDeviceToHost));
    const size_t HW = (size_t)ctx->H * ctx->W;
    for (size_t p = 0; p < HW; ++p) out[p] = ((bits[p >> 5] >> (p & 31)) & 1u) ? 255 : 0;
    return VC_OK;
}

int vc_upload_frame(vc_ctx *ctx, uint32_t slot, uint32_t cam, const uint8_t *bgr)
{
    if (!ctx || !bgr) return VC_ERR_ARG;
    Slot *s = nullptr;
    VC_TRY(slot_at(ctx, slot, &s));
    if (cam >= ctx->C) return fail(ctx, VC_ERR_ARG, "camera %u not in [0,%u)", cam, ctx->C);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->H * ctx->W;
    VC_TRY(ensure(ctx, s->frames, npix * ctx->C));
    VC_TRY(ensure(ctx, s->fbytes[cam], npix * 3 + 64));
    VC_TRY(stage_upload(ctx, *s, s->h_fbytes[cam], s->fbytes[cam].ptr, bgr, npix * 3, false));
    s->have_frame[cam] = 1;
    s->frame_dirty[cam] = 1;
    s->bits_valid = false;           // the image expansion rides in the same launch as the bit-packing
    return VC_OK;
}

// The y-major table [C][n_pad] (+ the y-line words' boxes): what the streaming and the one-thread-per-voxel kernels, the
// y-line hierarchical kernel and vc_fetch_lut read.  The default kernels read the tile-ordered table only, so this one is
// built when something first asks for it (19 ms at 1024^3 x 4, 17 GB).
static int ensure_ymajor(vc_ctx *ctx)
{
    if (ctx->ymajor_valid) return VC_OK;
    const uint64_t n = ctx->n_voxels();
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    VC_TRY(ensure(ctx, ctx->d_lut, (size_t)n_pad * ctx->C));
    VC_TRY(ensure(ctx, ctx->d_bbox, (size_t)(n_pad / 64) * ctx->C));
    if (n) {
        CarveParams p;
        fill_params(ctx, p);
        if (ctx->lut_foreign && ctx->tile_valid) {               // a table that was handed in: permuted back, never re-projected
            hipLaunchKernelGGL(k_untile_lut, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, (const int32_t *)ctx->d_lut_tile.ptr, ctx->d_lut.ptr);
            hipLaunchKernelGGL(k_adopt_lut<false>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, (const int32_t *)ctx->d_lut.ptr,
                               ctx->d_lut.ptr, ctx->d_bbox.ptr);
        }
        else hipLaunchKernelGGL(k_build_lut<false>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, ctx->d_lut.ptr, ctx->d_bbox.ptr);
        VC_HIP(ctx, hipGetLastError());
    }
    ctx->bbox_valid = true;
    ctx->ymajor_valid = true;
    return VC_OK;
}

int vc_build_lut(vc_ctx *ctx)
{
    if (!ctx) return VC_ERR_ARG;
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->have_grid || !ctx->have_cams) return fail(ctx, VC_ERR_ARG, "grid and cameras must be set before vc_build_lut");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_voxels();
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    VC_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    ctx->tile_valid = false;
    ctx->lut_foreign = false; ctx->ymajor_valid = false; ctx->upload_mask = 0;
    drop_lut16(ctx);
    if (ctx->lut_tile && ctx->nx % 4 == 0 && ctx->ny % 64 == 0) {
        // ONE table, in tile order (words of 4 x-rows x 16 y), projected straight into that order; the colour look-up of
        // the record expansion reads it too (closed-form index).  No y-major copy unless something asks for one.
        VC_TRY(ensure(ctx, ctx->d_lut_tile, (size_t)n_pad * ctx->C));
        VC_TRY(ensure(ctx, ctx->d_tbox, (size_t)(n_pad / 64) * ctx->C));
        if (n) {
            CarveParams p;
            fill_params(ctx, p);
            hipLaunchKernelGGL(k_build_lut<true>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, ctx->d_lut_tile.ptr, ctx->d_tbox.ptr);
            VC_HIP(ctx, hipGetLastError());
            ctx->tile_valid = true;
            ctx->tbox_valid = true;
            VC_TRY(build_brick_boxes(ctx));
        }
    } else {
        VC_TRY(ensure_ymajor(ctx));
    }
    VC_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.lut_ms, ctx->ev[0], ctx->ev[1]));
    ctx->lut_valid = true;
    ctx->lut_foreign = false;
    return VC_OK;
}

// One camera's table from the host (the counterpart of vc_fetch_lut; reference: the pickled lookup table that
// assignment.py:12-15 loads).  When every camera has been handed in, the tables are adopted: permuted into tile order
// where the grid allows (the y-major copy is released again) and the word / brick boxes are reduced from them.
int vc_upload_lut(vc_ctx *ctx, uint32_t cam, const int32_t *lut)
{
    if (!ctx || !lut) return VC_ERR_ARG;
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->have_grid || !ctx->have_cams) return fail(ctx, VC_ERR_ARG, "grid and cameras must be set before vc_upload_lut");
    if (cam >= ctx->C) return fail(ctx, VC_ERR_ARG, "camera %u not in [0,%u)", cam, ctx->C);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_voxels();
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    drop_lut16(ctx);
    if (ctx->upload_mask == 0) {                                 // first camera of a new table: whatever was there is void
        ctx->lut_valid = false; ctx->ymajor_valid = false; ctx->tile_valid = false; ctx->bbox_valid = false; ctx->tbox_valid = false; ctx->kbox_valid = false;
        VC_TRY(ensure(ctx, ctx->d_lut, (size_t)n_pad * ctx->C));
        VC_HIP(ctx, hipMemsetAsync(ctx->d_lut.ptr, 0xff, (size_t)n_pad * ctx->C * sizeof(int32_t), ctx->stream));   // padding = -1
    }
    if (n) VC_HIP(ctx, hipMemcpyAsync(ctx->d_lut.ptr + (size_t)cam * n_pad, lut, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->upload_mask |= 1u << cam;
    if (ctx->upload_mask != (ctx->C >= 32 ? 0xffffffffu : (1u << ctx->C) - 1u)) return VC_OK;
    ctx->upload_mask = 0;
    CarveParams p;
    fill_params(ctx, p);
    if (ctx->lut_tile && ctx->nx % 4 == 0 && ctx->ny % 64 == 0) {
        VC_TRY(ensure(ctx, ctx->d_lut_tile, (size_t)n_pad * ctx->C));
        VC_TRY(ensure(ctx, ctx->d_tbox, (size_t)(n_pad / 64) * ctx->C));
        if (n) {
            hipLaunchKernelGGL(k_adopt_lut<true>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, (const int32_t *)ctx->d_lut.ptr,
                               ctx->d_lut_tile.ptr, ctx->d_tbox.ptr);
            VC_HIP(ctx, hipGetLastError());
            ctx->tile_valid = true;
            ctx->tbox_valid = true;
            VC_TRY(build_brick_boxes(ctx));
        }
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->d_lut.reset();                                      // one table, as after vc_build_lut
    } else {
        VC_TRY(ensure(ctx, ctx->d_bbox, (size_t)(n_pad / 64) * ctx->C));
        if (n) {
            // (y-major path: the table stays where it is, so entries outside [-1, H*W) are rewritten to -1 IN PLACE)
            hipLaunchKernelGGL(k_adopt_lut<false>, dim3(grid_for(n_pad)), dim3(kBlock), 0, ctx->stream, p, (const int32_t *)ctx->d_lut.ptr,
                               ctx->d_lut.ptr, ctx->d_bbox.ptr);
            VC_HIP(ctx, hipGetLastError());
        }
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->bbox_valid = true;
        ctx->ymajor_valid = true;
    }
    ctx->lut_valid = true;
    ctx->lut_foreign = true;
    return VC_OK;
}

int vc_fetch_lut(vc_ctx *ctx, uint32_t cam, int32_t *out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    if (!ctx->lut_valid) return fail(ctx, VC_ERR_ARG, "no lookup table: call vc_build_lut");
    if (cam >= ctx->C) return fail(ctx, VC_ERR_ARG, "camera %u not in [0,%u)", cam, ctx->C);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(ensure_ymajor(ctx));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t n = ctx->n_voxels();
    const uint64_t n_pad = (n + kLutPad - 1) / kLutPad * kLutPad;
    if (n) VC_HIP(ctx, hipMemcpy(out, ctx->d_lut.ptr + (size_t)cam * n_pad, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_project(vc_ctx *ctx, uint32_t cam, const double *xyz, uint64_t n, double *uv)
{
    if (!ctx || !xyz || !uv) return VC_ERR_ARG;
    if (!ctx->have_cams || cam >= ctx->C) return fail(ctx, VC_ERR_ARG, "camera %u not set", cam);
    if (n == 0) return VC_OK;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(ensure(ctx, ctx->d_scratch, (size_t)n * 5));
    double *d_xyz = ctx->d_scratch.ptr, *d_uv = d_xyz + 3 * n;
    VC_HIP(ctx, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_project, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, ctx->cams[cam], d_xyz, n, d_uv);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(uv, d_uv, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VC_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the carve step
// What the three entry points ask of step_begin.  sync: the step is collected at once (vc_carve, vc_carve_footprint), events between
// its kernels cost nothing that matters.  foot_rule != 0: the carve kernel is k_carve_foot with this rule and q.
struct StepRequest { uint32_t slot, min_views; int color_cam, mode; uint32_t flags; bool sync; uint32_t foot_rule, foot_q; };
struct StepSize { uint64_t n, nwords; uint32_t ngroups, nscan; };

static bool stages_grids(Carve f) { return f >= Carve::FusedHier; }
// scan and record expansion run beside the next step's carve | packing and collectives of a rank do
static hipStream_t emit_stream(const vc_ctx *ctx) { return (ctx->overlap && !ctx->comm) ? ctx->stream2 : ctx->stream; }
static hipStream_t exchange_stream(const vc_ctx *ctx) { return ctx->overlap ? ctx->stream_x : ctx->stream; }

// The route, first half: what follows from the request and the context as the step finds it -- grid shape, C, mwords, the options,
// tile_valid / ymajor_valid, tile_whole.  Where the carve reads the y-major table (carve_table), ensure_ymajor runs in front of
// it and leaves ymajor_valid set: the expansion's table and the compact table's test are decided HERE as they stand BEHIND that call.
// Left open: Bricks or k_cull, which wait for ensure_boxes (settle_route), and the LDS of the grid-staging families (step_prepare).
static StepRoute plan_route(const vc_ctx *ctx, const StepRequest &rq, bool tile_whole)
{
    StepRoute r;
    const bool foot = rq.foot_rule != 0, no_records = (rq.flags & VC_FLAG_NO_RECORDS) != 0;
    r.lut = rq.mode == VC_MODE_LUT; r.viewmask = (rq.flags & VC_FLAG_VIEWMASK) != 0;
    r.allseen = foot || rq.min_views == ctx->C;
    // The chunked kernels cover the reference's case (seen by ALL cameras); the one-thread-per-voxel kernels cover thresholds below C, the
    // camera bitmask, and thresholds above C (no voxel can be seen by more cameras than there are: the reference's
    // sum(views.values()) >= views_threshold is never true, the result is empty) -- and masks too large for k_lut_first's LDS (one camera's)
    bool fast = !foot && !ctx->force_generic && !r.viewmask && rq.min_views == ctx->C;
    if (r.lut && !ctx->lut_hier && (size_t)ctx->mwords * sizeof(uint32_t) > kMaxFirstLds) fast = false;
    r.grids = fast;
    if (foot) r.family = Carve::Foot;
    else if (!fast) r.family = Carve::Generic;
    else if (r.lut && ctx->lut_hier) {
        r.family = Carve::LutHier;
        r.tile = ctx->lut_tile && ctx->tile_valid;
        r.pair = ctx->refine_pair != 0; r.b16 = !r.pair && ctx->refine_b != 8;
    }
    else if (r.lut) { r.family = Carve::LutStream; r.b16 = ctx->refine_b != 8; r.lds = (size_t)ctx->mwords * sizeof(uint32_t); }
    else if (ctx->ny % 64 == 0 && ctx->fused_hier) {
        r.family = Carve::FusedHier;
        r.tile = ctx->fused_tile && ctx->nx % 4 == 0;                 // ny % 64 == 0 here
        r.boxes = ctx->fused_boxes ? 2 : ctx->fused_f32box ? 1 : 0;
    }
    else r.family = Carve::FusedChunked;
    const bool hier = stages_grids(r.family);
    r.boxed_tiles = hier && r.tile && (r.lut || r.boxes == 2);
    r.zero_counts = hier && r.tile && !tile_whole;
    r.sparse_words = hier && !r.zero_counts;
    r.counted = hier || r.family == Carve::LutStream;                 // (chunked, one thread per voxel, footprint: their totals get counted)
    // which table the carve reads: the tile-ordered one (hierarchical kernel on tile words), else the y-major one
    r.carve_table = !r.lut ? Table::None : r.family == Carve::LutHier && r.tile ? Table::Tile : Table::YMajor;
    const bool ymajor = ctx->ymajor_valid || r.carve_table == Table::YMajor;
    if (rq.color_cam >= 0) {
        if (r.lut) r.emit_table = ctx->tile_valid && !ymajor ? Table::Tile : Table::YMajor;   // Tile: the only table there is
        else if (ctx->fused_color_table && !no_records) r.emit_table = Table::Color;
    }
    // the compact table: where the tile-ordered table is what the expansion reads and a group's tile words are 64 in a row.  (A step with a
    // threshold below C takes the one-thread-per-voxel carve and, from then on, the y-major table it builds: allseen holds wherever this applies.)
    r.try_lut16 = r.emit_table == Table::Tile && ctx->emit_lut16 && ctx->emit_lanes && !no_records && tile_whole && r.allseen;
    return r;
}

// The route, second half, behind ensure_boxes(tile) -- which sets kbox_valid for the table-free tile route: the brick pipeline
// where the shape allows, else k_cull in front of the one-launch kernel; and what hangs on that: the busy list and the events.
static void settle_route(const vc_ctx *ctx, const StepRequest &rq, bool carve_timed, bool tile_whole, uint32_t ngroups, StepRoute &r)
{
    const bool no_records = (rq.flags & VC_FLAG_NO_RECORDS) != 0;
    if (r.boxed_tiles && brick_shape(ctx)) {
        r.family = Carve::Bricks;
        r.wide_grids = r.sparse_words = true;                         // (k_cull_bricks zeroes every group's count itself)
    }
    else if (r.boxed_tiles) r.cull = ctx->cull && ctx->kbox_valid;
    // a rank of a communicator packs and exchanges the counts right behind the carve: vc_allgather finds them on the host
    r.exchange = no_records && ctx->comm && ctx->gather_compact;
    r.count_nz = r.exchange && r.family == Carve::Bricks && tile_whole;
    // the expansion of a large grid iterates over the scan's list of groups that have survivors (a rank's packing strides over it too)
    r.busy = ctx->emit_lanes && (!no_records || (r.exchange && r.count_nz)) &&
             (ctx->emit_busy == 2 || (ctx->emit_busy == 1 && ngroups >= kBusyListMinGroups));
    // the events a pipelined step hands from stream to stream ride on the launches in front: {scan done} on k_finish_scan, {step done} on the expansion
    r.xstream = r.exchange && exchange_stream(ctx) != ctx->stream;   // the packing waits for the scan across streams
    r.scan_ev = (!no_records && (emit_stream(ctx) != ctx->stream || carve_timed)) || r.xstream;
    r.ride = ctx->launch_events && !no_records;
    r.scan_ridden = r.busy && ctx->launch_events && r.scan_ev;
}

// vc_ctx::kev_sb names the step whose kernels are being queued for as long as step_begin runs, whichever way it leaves
struct KevScope { vc_ctx *ctx; ~KevScope() { ctx->kev_sb = nullptr; } };

// Stage 1 (behind the refusals): the step's set of buffers, its events from the ring, the result it replaces invalidated ...
static StepBuf &step_open(vc_ctx *ctx, const StepRequest &rq)
{
    ctx->gathered = false;
    result_changed(ctx);   // the next carve invalidates what the post-carve passes left
    ctx->tm.voxels = ctx->n_voxels();
    if (ctx->head == ctx->cur) {
        // this step is queued into the buffers that hold the result the vc_fetch_* functions read: it is gone from here on
        ctx->carved = false; ctx->viewmask_valid = false; ctx->packed = false;
    }
    StepBuf &sb = ctx->sb[ctx->head];
    Event *ev = ctx->step_ev[ctx->step_next];
    sb.e_scan = ev[0]; sb.e2 = ev[1]; sb.e_emit0 = ev[2];
    ctx->step_next = (ctx->step_next + 1) % kStepRing;
    sb.n = ctx->n_voxels(); sb.survivors = 0; sb.kmask = 0;
    sb.min_views = rq.min_views; sb.color_cam = rq.color_cam; sb.slot = rq.slot;
    sb.no_records = (rq.flags & VC_FLAG_NO_RECORDS) != 0;
    sb.sparse_words = sb.counts_exchanged = false;
    sb.carve_timed = ctx->timing_detail || rq.sync;
    if (ctx->timing_detail || ctx->kernel_events) ctx->kev_sb = &sb;   // every launch of this step carries begin / end events
    return sb;
}

// ... and the empty slab, which still takes part in the collective
static int step_empty(vc_ctx *ctx, StepBuf &sb)
{
    if (sb.no_records && ctx->comm && ctx->gather_compact) {
        hipStream_t sx = exchange_stream(ctx);
        VC_TRY(enqueue_pack(ctx, sb, sx));
        VC_TRY(enqueue_counts_exchange(ctx, sb, sx));
        VC_HIP(ctx, hipEventRecord(sb.e2, sx));
        sb.counts_exchanged = true;
    }
    sb.pending = true; sb.used = false; ctx->head = (ctx->head + 1) % kDepth; ctx->npending++;
    return VC_OK;
}

// Stage 2: the step's buffers (timing_detail: and the kernels' work counters), and the carve's pointers into them
static int step_size(vc_ctx *ctx, const StepRequest &rq, StepBuf &sb, const StepSize &z, CarveParams &p)
{
    VC_TRY(ensure(ctx, sb.words, p.n_pad / 64));
    VC_TRY(ensure(ctx, sb.groupcnt, z.ngroups)); VC_TRY(ensure(ctx, sb.groupoff, z.ngroups));
    VC_TRY(ensure(ctx, sb.blocksum, kMaxScanBlocks)); VC_TRY(ensure(ctx, sb.blockoff, kMaxScanBlocks + 1));
    if (rq.flags & VC_FLAG_VIEWMASK) VC_TRY(ensure(ctx, ctx->d_viewmask, z.n));
    if (!sb.records.ptr && !sb.no_records) VC_TRY(ensure(ctx, sb.records, (size_t)(z.n / 16 + 1024)));
    if (ctx->timing_detail) {
        if (!ctx->d_stats.ptr) {
            VC_TRY(ensure(ctx, ctx->d_stats, (size_t)VC_WORK_KINDS * kShards * kStatStride));
            VC_HIP(ctx, hipMemset(ctx->d_stats.ptr, 0, ctx->d_stats.cap * sizeof(unsigned long long)));
        }
        p.stats = ctx->d_stats.ptr;
    }
    p.words = sb.words.ptr; p.groupcnt = sb.groupcnt.ptr; p.viewmask = ctx->d_viewmask.ptr; p.min_views = rq.min_views;
    return VC_OK;
}

// Stage 4: everything that is made in front of the carve, in this order.  The tables sit HERE, on the carve stream in front of the carve
// kernels, so that {scan done} -- which the expansion waits for on its own stream and which rides on the k_finish_scan launch -- is behind
// them: queued where the expansion's parameters are set up, they would follow that launch and the first expansion read a table being written.
static int step_prepare(vc_ctx *ctx, const StepRequest &rq, StepBuf &sb, Slot &s, const StepSize &z, CarveParams &p)
{
    StepRoute &r = sb.route;
    if (r.boxed_tiles && !r.lut) VC_TRY(ensure_boxes(ctx, true));         // tile boxes without a table (and the brick boxes behind them)
    settle_route(ctx, rq, sb.carve_timed, p.tile_whole != 0, z.ngroups, r);
    sb.sparse_words = r.sparse_words;
    // per-frame preparation (nothing to do when the slot has been used before); it sizes the grids for the LDS of the kernels that stage them
    sb.prepped = !s.bits_valid || (r.grids && !s.grids_valid);
    sb.prep_timed = sb.prepped && sb.carve_timed;
    VC_TRY(ensure_prepared(ctx, s, r.grids, &p, sb.prep_timed, r.wide_grids));
    if (stages_grids(r.family)) r.lds = ((size_t)s.budget_words + 8) * sizeof(uint32_t);
    sb.nz_valid = r.count_nz;
    if (r.count_nz) {
        VC_TRY(ensure(ctx, sb.groupnz, z.ngroups));
        p.groupnz = sb.groupnz.ptr;
    }
    sb.slot_gen = s.gen;
    if (s.prep_pending) { VC_HIP(ctx, hipStreamWaitEvent(ctx->stream, s.e_prep, 0)); s.prep_pending = false; }
    if (r.family == Carve::Foot) VC_TRY(ensure_footprint(ctx, s));         // lattices + the slot's tables, behind the preparation
    p.maskbits = s.bits.ptr; p.blockgrid = s.grid.ptr; p.coarsegrid = s.has_coarse ? s.coarse.ptr : nullptr;
    p.counts = s.boxes.ptr + kCountBase;
    if (r.carve_table == Table::YMajor) VC_TRY(ensure_ymajor(ctx));
    p.lut = ctx->d_lut.ptr; p.bbox = ctx->d_bbox.ptr;
    // the colour camera's table over the whole grid (VC_MODE_FUSED), its compact tile-ordered table (VC_MODE_LUT): made by the first step that names it
    if (r.emit_table == Table::Color) VC_TRY(ensure_color_table(ctx, rq.color_cam));
    if (r.try_lut16) VC_TRY(ensure_lut16(ctx, rq.color_cam, p.n_pad, r.lut16));
    return VC_OK;
}

// Stage 5: the carve kernels of the route, between the step's timing events
static int step_carve(vc_ctx *ctx, const StepRequest &rq, StepBuf &sb, Slot &s, const StepSize &z, CarveParams &p)
{
    const StepRoute &r = sb.route;
    const dim3 block(kBlock);
    // grids of the kernels whose workgroups stride: four waves' items per workgroup, so many workgroups per CU at the most
    auto strided = [](uint64_t items, int per_cu) {
        const uint64_t want = (items + 3) / 4, most = 256ull * (uint64_t)per_cu;
        return dim3((uint32_t)(want < most ? want : most));
    };
    const uint64_t groups = p.n_pad / 4096;
#define VC_CARVE(kernel, grid, blk, lds) VC_KLAUNCH(VC_K_CARVE_ONE_LAUNCH, kernel, grid, blk, lds, ctx->stream, p)
    if (sb.carve_timed) VC_HIP(ctx, hipEventRecord(sb.e0, ctx->stream));
    if (r.zero_counts) VC_HIP(ctx, hipMemsetAsync(sb.groupcnt.ptr, 0, sizeof(uint32_t) * z.ngroups, ctx->stream));
    if (r.boxed_tiles && !r.lut) { p.tbox = ctx->d_tbox.ptr; p.kbox = ctx->d_kbox.ptr; }     // (ensure_boxes may have made them)
    if (r.cull) {
        p.live = ctx->d_live.ptr;
        const uint32_t cw = p.nbrick_pad / 256;
        VC_KLAUNCH(VC_K_CULL, k_cull, dim3(cw < 1 ? 1 : (cw > 1024 ? 1024 : cw)), block, r.lds, ctx->stream, p);
    }
    switch (r.family) {
    case Carve::Foot: {
        FootParams f;
        f.lx = ctx->d_foot_axes.ptr; f.ly = f.lx + ctx->nx + 1; f.lz = f.ly + ctx->ny + 1;
        f.sat = s.sat.ptr; f.rule = rq.foot_rule; f.q = rq.foot_q;
        const dim3 grid((uint32_t)((z.nwords + 3) / 4));
        if (r.viewmask) VC_KLAUNCH(VC_K_FOOT_CARVE, (k_carve_foot<true>), grid, block, 0, ctx->stream, p, f);
        else VC_KLAUNCH(VC_K_FOOT_CARVE, (k_carve_foot<false>), grid, block, 0, ctx->stream, p, f);
        break;
    }
    case Carve::Generic: {
        const dim3 grid(grid_for(z.n));
        if (r.lut && r.viewmask) VC_CARVE((k_carve_generic<true, true>), grid, block, 0);
        else if (r.lut) VC_CARVE((k_carve_generic<true, false>), grid, block, 0);
        else if (r.viewmask) VC_CARVE((k_carve_generic<false, true>), grid, block, 0);
        else VC_CARVE((k_carve_generic<false, false>), grid, block, 0);
        break;
    }
    case Carve::FusedChunked: {
        const dim3 grid = strided((z.n + 64 * kSub - 1) / (64 * kSub), ctx->fused_blocks_per_cu);
        if (ctx->ny % 64 == 0) VC_CARVE((k_carve_fused<kSub, true>), grid, block, 0);
        else VC_CARVE((k_carve_fused<kSub, false>), grid, block, 0);
        break;
    }
    case Carve::LutStream: {
        const int kv = ctx->first_kv;
        const uint64_t fwant = (p.n_pad / (256 * kv) + 7) / 8;
        uint32_t per_cu = (uint32_t)(kLdsBytes / (r.lds ? r.lds : 1));
        if (per_cu > (uint32_t)ctx->first_blocks_per_cu) per_cu = (uint32_t)ctx->first_blocks_per_cu;
        const uint32_t fmax = 256u * (per_cu < 1 ? 1u : per_cu);
        const dim3 fgrid((uint32_t)(fwant < fmax ? fwant : fmax)), fblock(kFirstBlock);
        if (kv == 1) VC_CARVE((k_lut_first<1>), fgrid, fblock, r.lds);
        else if (kv == 4) VC_CARVE((k_lut_first<4>), fgrid, fblock, r.lds);
        else VC_CARVE((k_lut_first<2>), fgrid, fblock, r.lds);
        VC_HIP(ctx, hipGetLastError());
        if (sb.carve_timed) VC_HIP(ctx, hipEventRecord(sb.e_first, ctx->stream));
        const dim3 rgrid = strided(groups, ctx->refine_blocks_per_cu);
        if (!r.b16) VC_CARVE((k_lut_refine<8, false, false>), rgrid, block, 0);
        else VC_CARVE((k_lut_refine<16, false, false>), rgrid, block, 0);
        break;
    }
    case Carve::FusedHier: {                     // word-level rejection by interval arithmetic, or by the boxes read
        const dim3 rgrid = strided(groups, ctx->hier_blocks_per_cu);
        if (!r.tile && r.boxes == 2) {           // (the y-line boxes: built by the first such step, behind its first timing event)
            VC_TRY(ensure_boxes(ctx, false));
            p.bbox = ctx->d_bbox.ptr;
        }
        if (r.tile && r.boxes == 2) VC_CARVE((k_carve_fused_hier<true, 2>), rgrid, block, r.lds);
        else if (r.tile && r.boxes == 1) VC_CARVE((k_carve_fused_hier<true, 1>), rgrid, block, r.lds);
        else if (r.tile) VC_CARVE((k_carve_fused_hier<true, 0>), rgrid, block, r.lds);
        else if (r.boxes == 2) VC_CARVE((k_carve_fused_hier<false, 2>), rgrid, block, r.lds);
        else if (r.boxes == 1) VC_CARVE((k_carve_fused_hier<false, 1>), rgrid, block, r.lds);
        else VC_CARVE((k_carve_fused_hier<false, 0>), rgrid, block, r.lds);
        break;
    }
    case Carve::LutHier: {                       // one launch: word-level rejection by pixel box x foreground-block grid, exact test for the rest
        const dim3 rgrid = strided(groups, ctx->hier_blocks_per_cu);
        if (r.tile) VC_CARVE((k_lut_refine<8, true, true, true>), rgrid, block, r.lds);
        else if (r.pair) VC_CARVE((k_lut_refine<8, true, true>), rgrid, block, r.lds);
        else if (!r.b16) VC_CARVE((k_lut_refine<8, true, false>), rgrid, block, r.lds);
        else VC_CARVE((k_lut_refine<16, true, false>), rgrid, block, r.lds);
        break;
    }
    case Carve::Bricks:
        if (r.lut) VC_TRY(launch_bricks<true>(ctx, p, r.lds, z.ngroups));
        else VC_TRY(launch_bricks<false>(ctx, p, r.lds, z.ngroups));
        break;
    }
#undef VC_CARVE
    VC_HIP(ctx, hipGetLastError());
    if (sb.carve_timed) VC_HIP(ctx, hipEventRecord(sb.e1, ctx->stream));
    return VC_OK;
}

// Stage 6: group counts -> two-level scan (and the list of busy groups), on the carve stream right behind the carve: on the expansion's
// stream the small scan kernels would queue for compute units against the next carve's thousands of workgroups and delay the expansion
static int step_scan(vc_ctx *ctx, StepBuf &sb, const StepSize &z)
{
    const StepRoute &r = sb.route;
    hipStream_t st = ctx->stream;
    const dim3 block(kBlock);
    if (!r.counted) {
        VC_KLAUNCH(VC_K_COUNT_GROUPS, k_count_groups, dim3((z.ngroups + 3) / 4), block, 0, st, sb.words.ptr, z.nwords, z.ngroups,
                           sb.groupcnt.ptr);
        VC_HIP(ctx, hipGetLastError());
    }
    if (r.busy) {
        VC_TRY(ensure(ctx, sb.busyoff, z.ngroups)); VC_TRY(ensure(ctx, sb.busylist, z.ngroups));
        VC_TRY(ensure(ctx, sb.busysum, kMaxScanBlocks)); VC_TRY(ensure(ctx, sb.busyblock, 1));   // (busyblock: the count of busy groups)
    }
    VC_KLAUNCH(VC_K_SCAN_GROUPS, k_scan_groups, dim3(z.nscan), dim3(kScanThreads), 0, st, (const uint32_t *)sb.groupcnt.ptr, z.ngroups, sb.groupoff.ptr,
               sb.blocksum.ptr, sb.blockoff.ptr, sb.h_total.ptr, r.busy ? sb.busyoff.ptr : (uint32_t *)nullptr, sb.busysum.ptr,
               sb.busyblock.ptr, (uint32_t)ctx->dbg);
    VC_HIP(ctx, hipGetLastError());
    if (r.busy) {
        // level 2 of both scans + the list in one launch (k_scan_groups has left the count in busyblock[0] when nscan == 1)
        hipEvent_t fs0 = nullptr, fs1 = nullptr;
        kev_pick(ctx, VC_K_FINISH_SCAN, fs0, fs1);
        if (r.scan_ridden) { fs1 = sb.e_scan; if (fs0) sb.kused[VC_K_FINISH_SCAN][1] = fs1; }
        hipExtLaunchKernelGGL(k_finish_scan, dim3(grid_for(z.ngroups)), block, 0, st, fs0, fs1, 0,
                              (const uint64_t *)sb.blocksum.ptr, z.nscan, sb.blockoff.ptr, sb.h_total.ptr, (const uint32_t *)sb.busysum.ptr, sb.busyblock.ptr,
                              (const uint32_t *)sb.groupcnt.ptr, z.ngroups, (const uint32_t *)sb.busyoff.ptr, sb.busylist.ptr, (uint32_t)ctx->dbg);
        VC_HIP(ctx, hipGetLastError());
    } else if (z.nscan > 1) {
        hipLaunchKernelGGL(k_scan_blocks, dim3(1), dim3(kScanThreads), 0, st, sb.blocksum.ptr, z.nscan, sb.blockoff.ptr, sb.h_total.ptr);
        VC_HIP(ctx, hipGetLastError());
    }
    return VC_OK;
}

// Stage 7: the expansion's parameters (kept with the step for a re-run after a records regrow)
static void step_emit_params(const vc_ctx *ctx, StepBuf &sb, const StepSize &z, const CarveParams &p)
{
    const StepRoute &r = sb.route;
    EmitParams &e = sb.emit;
    emit_color_source(ctx, sb.slot, sb.color_cam, e);
    e.words = sb.words.ptr; e.groupcnt = sb.groupcnt.ptr; e.groupoff = sb.groupoff.ptr; e.blockoff = sb.blockoff.ptr;
    e.n = z.n; e.i0 = ctx->i0(); e.ngroups = z.ngroups; e.z0 = ctx->z0;
    if (r.emit_table == Table::Tile) {
        e.lut = ctx->d_lut_tile.ptr + (size_t)sb.color_cam * p.n_pad;
        e.lut_tq = p.tq;
        if (r.lut16) { e.lut16 = ctx->d_lut16.ptr; e.cbase = ctx->d_cbase.ptr; }   // ... and its compact form
    }
    else if (r.emit_table == Table::YMajor) e.lut = ctx->d_lut.ptr + (size_t)sb.color_cam * p.n_pad;
    // (table-free carve, but the survivors' colour look-up reads the colour camera's table instead of projecting each of them again)
    else if (r.emit_table == Table::Color) e.lut = ctx->d_lut_color.ptr + ctx->i0();
    e.records = sb.records.ptr; e.capacity = sb.records.cap;
    e.busylist = sb.busylist.ptr; e.busycount = sb.busyblock.ptr;
    e.dbg = (uint32_t)ctx->dbg; e.stats = p.stats;
}

// Stage 8: the record expansion on its stream (memory bound where the carve kernels are VALU-issue bound: it runs beside the carve of
// the next step, two steps in flight), a rank's packing and exchange on theirs, and the step's events handed to the slot
static int step_finish(vc_ctx *ctx, StepBuf &sb, Slot &s)
{
    const StepRoute &r = sb.route;
    hipStream_t s3 = emit_stream(ctx), sx = exchange_stream(ctx);
    sb.emit_ridden = r.ride;
    sb.emit_timed = false;
    if (r.scan_ev) {
        if (!r.scan_ridden) VC_HIP(ctx, hipEventRecord(sb.e_scan, ctx->stream));     // cross-stream dependency
        if (!sb.no_records && s3 != ctx->stream) VC_HIP(ctx, hipStreamWaitEvent(s3, sb.e_scan, 0));
        if (r.xstream) VC_HIP(ctx, hipStreamWaitEvent(sx, sb.e_scan, 0));
        sb.emit_timed = !sb.no_records;
    }
    if (!sb.no_records) {
        VC_TRY(launch_emit(ctx, sb, s3, r.ride ? sb.e_emit0 : nullptr, r.ride ? sb.e2 : nullptr));
        if (r.ride) sb.emit_timed = true;
    }
    if (r.exchange) {
        VC_TRY(enqueue_pack(ctx, sb, sx));
        VC_TRY(enqueue_counts_exchange(ctx, sb, sx));
        sb.counts_exchanged = true;
    }
    if (!r.ride || r.exchange) VC_HIP(ctx, hipEventRecord(sb.e2, r.exchange ? sx : sb.no_records ? ctx->stream : s3));
    if (!sb.no_records && s3 != ctx->stream) { s.e_emit = sb.e2; s.emit_pending = true; }   // the expansion reads the slot's bits / images
    // ... and, table-free with a colour camera, the one whole-grid colour table: a later step that names another camera waits
    if (!sb.no_records && s3 != ctx->stream && r.emit_table == Table::Color) ctx->lut_color_reader = sb.e2;
    // the slot's next preparation waits for the kernels of THIS step that read its bits / grids: always this step's own event (a flag left set by
    // an earlier step on the slot must not keep that step's event in place: the preparation would then overwrite bits and grids under this
    // step's carve).  Without e_scan, e2 is behind the carve kernels too.
    s.e_carve = r.scan_ev ? sb.e_scan : sb.e2;
    s.carve_pending = true;
    sb.pending = sb.used = true; ctx->head = (ctx->head + 1) % kDepth; ctx->npending++;
    return VC_OK;
}

// A step, stage by stage
static int step_begin(vc_ctx *ctx, StepRequest rq)
{
    if (!ctx) return VC_ERR_ARG;
    if (ctx->npending >= kDepth) return fail(ctx, VC_ERR_ARG, "%d carve steps are already in flight: call vc_carve_end", kDepth);
    if (!ctx->have_grid || !ctx->have_cams) return fail(ctx, VC_ERR_ARG, "grid and cameras must be set before vc_carve");
    if (rq.slot >= ctx->slots.size() || !ctx->slots[rq.slot].have_masks)
        return fail(ctx, VC_ERR_ARG, "no masks uploaded in slot %u", rq.slot);
    if (rq.mode != VC_MODE_FUSED && rq.mode != VC_MODE_LUT) return fail(ctx, VC_ERR_ARG, "unknown mode %d", rq.mode);
    if (rq.mode == VC_MODE_LUT && !ctx->lut_valid) return fail(ctx, VC_ERR_ARG, "VC_MODE_LUT needs vc_build_lut first");
    if (rq.color_cam >= (int)ctx->C) return fail(ctx, VC_ERR_ARG, "colour camera %d not in [0,%u)", rq.color_cam, ctx->C);
    if (rq.min_views < 1) rq.min_views = 1;      // a voxel no camera sees never enters voxels_visible
    VC_HIP(ctx, hipSetDevice(ctx->device));
    KevScope scope{ctx};
    StepBuf &sb = step_open(ctx, rq);                                      // 1
    CarveParams p;
    fill_params(ctx, p);
    sb.route = plan_route(ctx, rq, p.tile_whole != 0);                     // 3, first half (an empty slab keeps it too: mode, allseen, view masks)
    if (sb.n == 0) return step_empty(ctx, sb);
    Slot &s = ctx->slots[rq.slot];
    const uint32_t ngroups = (uint32_t)(p.n_pad / (64 * kGroupWords));
    const StepSize z{sb.n, (sb.n + 63) / 64, ngroups, (ngroups + kScanBlock - 1) / kScanBlock};
    VC_TRY(step_size(ctx, rq, sb, z, p));                                  // 2
    VC_TRY(step_prepare(ctx, rq, sb, s, z, p));                            // 4, with the route's second half behind the boxes
    VC_TRY(step_carve(ctx, rq, sb, s, z, p));                              // 5
    VC_TRY(step_scan(ctx, sb, z));                                         // 6
    step_emit_params(ctx, sb, z, p);                                       // 7
    return step_finish(ctx, sb, s);                                        // 8
}

int vc_carve_begin(vc_ctx *ctx, uint32_t slot, uint32_t min_views, int color_cam, int mode, uint32_t flags)
{
    return step_begin(ctx, StepRequest{slot, min_views, color_cam, mode, flags, false, 0, 0});
}

// Completes the oldest step in flight: its survivor count, and its records become what the
// vc_fetch_* functions and vc_allgather read.
int vc_carve_end(vc_ctx *ctx, uint64_t *n_out)
{
    if (!ctx || !n_out) return VC_ERR_ARG;
    *n_out = 0;
    if (ctx->npending == 0) return fail(ctx, VC_ERR_ARG, "no carve step in flight");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const int k = (ctx->head - ctx->npending + kDepth) % kDepth;           // oldest pending set
    StepBuf &sb = ctx->sb[k];
    ctx->carved = false; ctx->viewmask_valid = false; ctx->gathered = false; ctx->packed = false; result_changed(ctx);
    if (sb.n != 0) {
        VC_HIP(ctx, hipEventSynchronize(sb.e2));
        uint64_t total = *sb.h_total;
        if (!sb.no_records && total > sb.records.cap) {                    // regrow once, expand again
            // the second expansion reads the step's frame set (bits, image) NOW: if a later vc_carve_begin has prepared the slot
            // again in the meantime, colours and seen flags would come from the newer frame -- refuse instead of mixing
            if (sb.color_cam >= 0 && ctx->slots[sb.slot].gen != sb.slot_gen) {
                sb.pending = false; ctx->npending--;
                return fail(ctx, VC_ERR_ARG, "step overflowed its record buffer (%llu > %llu) and frame set %u has been prepared again "
                            "since: its records cannot be re-expanded; collect a step before re-using its slot with new input",
                            (unsigned long long)total, (unsigned long long)sb.records.cap, sb.slot);
            }
            VC_TRY(ensure(ctx, sb.records, (size_t)(total + total / 8 + 1024)));
            sb.emit.records = sb.records.ptr;
            sb.emit.capacity = sb.records.cap;
            // (a later step may have packed the compact table for another colour camera since: d_lut_tile still holds this one's)
            if (sb.route.lut16 && ctx->lut16_cam != sb.color_cam) { sb.emit.lut16 = nullptr; sb.emit.cbase = nullptr; }
            // (... or projected the whole-grid colour table for another camera: a table-free step then projects its survivors
            // itself, as with fused_color_table = 0 -- the same bytes, and the table stays the newer step's)
            if (sb.route.emit_table == Table::Color && ctx->lut_color_cam != sb.color_cam) sb.emit.lut = nullptr;
            VC_TRY(launch_emit(ctx, sb, ctx->stream));
            sb.emit_ridden = false;
            VC_HIP(ctx, hipEventRecord(sb.e2, ctx->stream));
            VC_HIP(ctx, hipEventSynchronize(sb.e2));
        }
        sb.survivors = total;
        if (sb.carve_timed) {
            float ms = 0;
            VC_HIP(ctx, hipEventElapsedTime(&ms, sb.e0, sb.e1));
            ctx->tm.carve_ms = ms;
            ctx->tm.first_ms = ms;                               // one kernel sequence does the whole carve ...
            if (sb.route.family == Carve::LutStream) VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.first_ms, sb.e0, sb.e_first));   // ... unless a streaming first pass was timed
            ctx->tm.first_ms_sum += ctx->tm.first_ms;
            ctx->tm.carve_ms_sum += ms;
            ctx->tm.carve_launches += 1;
            VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.compact_ms, sb.e1, sb.e2));
        }
        if (sb.emit_timed) {
            // the launch's own begin .. end where they ride on it; else from {scan done}, which includes whatever the expansion
            // stream still had to finish first
            VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.emit_ms, sb.emit_ridden ? sb.e_emit0 : sb.e_scan, sb.e2));
            ctx->tm.emit_ms_sum += ctx->tm.emit_ms;
            ctx->tm.emit_launches += 1;
        }
        if (sb.emit_timed && sb.emit_ridden) { sb.kused[VC_K_EMIT][0] = sb.e_emit0; sb.kused[VC_K_EMIT][1] = sb.e2; sb.kmask |= 1u << VC_K_EMIT; }
        for (int kk = 0; kk < VC_KERNEL_KINDS; ++kk) {
            if (!((sb.kmask >> kk) & 1u)) continue;
            if (kk <= VC_K_PREP_GRID) VC_HIP(ctx, hipEventSynchronize(sb.kused[kk][1]));   // (upload stream: not ordered before e2 by itself)
            float ms = 0;
            if (hipEventElapsedTime(&ms, sb.kused[kk][0], sb.kused[kk][1]) == hipSuccess) {
                ctx->tm.kernel_ms_sum[kk] += ms;
                ctx->tm.kernel_launches[kk] += 1;
            }
        }
        sb.kmask = 0;
        ctx->tm.prep_ms = 0;
        if (sb.prepped) ctx->tm.preps += 1;
        if (sb.prep_timed) {
            Slot &sl = ctx->slots[sb.slot];
            VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.prep_ms, sl.e_p0, sl.e_prep));
            ctx->tm.prep_ms_sum += ctx->tm.prep_ms;
            ctx->tm.preps_timed += 1;
        }
    } else {
        if (sb.counts_exchanged) VC_HIP(ctx, hipEventSynchronize(sb.e2));
        sb.survivors = 0;
    }
    sb.pending = false;
    ctx->npending--;
    ctx->cur = k;
    ctx->survivors = sb.survivors;
    ctx->tm.survivors = sb.survivors;
    ctx->carved = true;
    ctx->viewmask_valid = sb.route.viewmask;
    *n_out = sb.survivors;
    return VC_OK;
}

int vc_carve(vc_ctx *ctx, uint32_t slot, uint32_t min_views, int color_cam, int mode, uint32_t flags,
             uint64_t *n_out)
{
    if (!ctx || !n_out) return VC_ERR_ARG;
    *n_out = 0;
    if (ctx->npending != 0) return fail(ctx, VC_ERR_ARG, "vc_carve with steps in flight: drain them with vc_carve_end");
    VC_TRY(step_begin(ctx, StepRequest{slot, min_views, color_cam, mode, flags, true, 0, 0}));
    return vc_carve_end(ctx, n_out);
}

// The footprint rule (include/voxcarve.h, csrc/vc_footprint.h): the synchronous step of vc_carve with k_carve_foot as its carve
// kernel.  Everything behind the words -- group counts, scan, record expansion, the result hand-over -- is the step's own.
int vc_carve_footprint(vc_ctx *ctx, uint32_t slot, uint32_t min_views, int color_cam, uint32_t rule, uint32_t q, uint32_t flags,
                       uint64_t *n_out)
{
    if (!ctx || !n_out) return VC_ERR_ARG;
    *n_out = 0;
    if (ctx->npending != 0) return fail(ctx, VC_ERR_ARG, "vc_carve_footprint with steps in flight: drain them with vc_carve_end");
    if (rule != VC_FOOT_ANY && rule != VC_FOOT_COVER) return fail(ctx, VC_ERR_ARG, "unknown footprint rule %u (VC_FOOT_ANY, VC_FOOT_COVER)", rule);
    if (rule == VC_FOOT_COVER && (q < 1 || q > 256)) return fail(ctx, VC_ERR_ARG, "footprint cover q = %u not in 1..256", q);
    if (flags & ~(uint32_t)(VC_FLAG_VIEWMASK | VC_FLAG_NO_RECORDS)) return fail(ctx, VC_ERR_ARG, "unknown flags 0x%x", flags);
    VC_TRY(step_begin(ctx, StepRequest{slot, min_views, color_cam, VC_MODE_FUSED, flags, true, rule, rule == VC_FOOT_COVER ? q : 1u}));
    return vc_carve_end(ctx, n_out);
}

// Page-locked host memory for the caller's output buffers: device-to-host copies into it run
// at PCIe rate instead of the pageable-memory rate (the reference has no counterpart; its
// outputs are Python lists).
int vc_host_alloc(vc_ctx *ctx, uint64_t bytes, void **out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    *out = nullptr;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return VC_OK;
}

int vc_host_free(vc_ctx *ctx, void *ptr)
{
    if (!ctx) return VC_ERR_ARG;
    if (ptr) VC_HIP(ctx, hipHostFree(ptr));
    return VC_OK;
}

int vc_fetch_records(vc_ctx *ctx, uint64_t *records)
{
    if (!ctx || !records) return VC_ERR_ARG;
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "no carve result to fetch");
    if (ctx->sb[ctx->cur].no_records)
        return fail(ctx, VC_ERR_ARG, "last carve ran with VC_FLAG_NO_RECORDS: use vc_allgather / vc_expand_entries");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->survivors)
        VC_HIP(ctx, hipMemcpy(records, ctx->sb[ctx->cur].records.ptr, ctx->survivors * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch(vc_ctx *ctx, uint32_t *idx, uint8_t *rgb, uint8_t *seen)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "no carve result to fetch");
    const uint64_t S = ctx->survivors;
    if (S == 0) return VC_OK;
    std::vector<uint64_t> rec(S);
    VC_TRY(vc_fetch_records(ctx, rec.data()));
    for (uint64_t k = 0; k < S; ++k) {
        const uint64_t r = rec[k];
        if (idx) idx[k] = (uint32_t)r;
        if (rgb) { rgb[3 * k] = (uint8_t)(r >> 32); rgb[3 * k + 1] = (uint8_t)(r >> 40); rgb[3 * k + 2] = (uint8_t)(r >> 48); }
        if (seen) seen[k] = (uint8_t)((r >> 56) & 1);
    }
    return VC_OK;
}

int vc_fetch_viewmask(vc_ctx *ctx, uint16_t *viewmask)
{
    if (!ctx || !viewmask) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->viewmask_valid) return fail(ctx, VC_ERR_ARG, "last carve did not keep the view mask (VC_FLAG_VIEWMASK)");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_voxels();
    if (n) VC_HIP(ctx, hipMemcpy(viewmask, ctx->d_viewmask.ptr, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

// The hierarchical kernels skip the words of groups without survivors (cur.sparse_words): their words are zeroed on the context's
// stream before anything reads the words whole.
static int densify_words(vc_ctx *ctx, StepBuf &cur)
{
    const uint64_t nwords = (ctx->n_voxels() + 63) / 64;
    if (!cur.sparse_words || !nwords) return VC_OK;
    const uint32_t ngroups = (uint32_t)((nwords + kGroupWords - 1) / kGroupWords);
    hipLaunchKernelGGL(k_zero_dead_groups, dim3((ngroups + 3) / 4), dim3(kBlock), 0, ctx->stream, cur.words.ptr, nwords, ngroups,
                       cur.groupcnt.ptr);
    VC_HIP(ctx, hipGetLastError());
    cur.sparse_words = false;
    return VC_OK;
}

int vc_fetch_occupancy(vc_ctx *ctx, uint8_t *bits)
{
    if (!ctx || !bits) return VC_ERR_ARG;
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "no carve result to fetch");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t nwords = (ctx->n_voxels() + 63) / 64;
    StepBuf &cur = ctx->sb[ctx->cur];
    if (cur.sparse_words) {
        VC_TRY(densify_words(ctx, cur));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (nwords) VC_HIP(ctx, hipMemcpy(bits, cur.words.ptr, nwords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

// after the call's stream has drained: the launches' times into vc_timing_t
static void dist_harvest(vc_ctx *ctx)
{
    for (size_t k = 0; k < ctx->dist_ev_kind.size(); ++k) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->dist_ev[2 * k], ctx->dist_ev[2 * k + 1]) == hipSuccess) {
            if (ctx->dist_ev_kind[k] == kThinKind) {             // (vc_hull_thin: no vc_kernel_kind, its own sum)
                ctx->tm.thin_kernel_ms += ms;
                ctx->tm.thin_launches += 1;
                continue;
            }
            ctx->tm.kernel_ms_sum[ctx->dist_ev_kind[k]] += ms;
            ctx->tm.kernel_launches[ctx->dist_ev_kind[k]] += 1;
        }
    }
    ctx->dist_ev_kind.clear();
}

// ---- the frame around a pass over the current carve result ----
// Every call that reads or rewrites the current result (colour, photo, components, distance, morphology, grow, render, surface
// mesh, normals, clusters, geodesic) keeps this order; the frame is the one place where it is written down:
//   pass_open    the refusals all passes share; hands back the step, S, n and nwords
//                (then the pass's own argument checks, in the order its contract gives them)
//   pass_begin   the host's side: device, a gather still in flight, the pinned scalars, no launch events left from a failed call
//                (then the pass drops its own stamp and sizes its buffers: nothing is queued yet, a failure leaves the result)
//   pass_start   the device's side: behind the step's record expansion, ev[0], the occupancy words whole
//                (then the pass's launches, memsets and copies)
//   pass_end     ev[1], the stream drained, the launches' own events harvested, the elapsed time
enum PassWords { kWordsLater, kWordsIfRecords, kWordsAlways };   // pass_start: who makes the occupancy words whole, and when

struct Pass {
    StepBuf *cur = nullptr;          // the step that holds the result
    uint64_t S = 0, n = 0, nwords = 0;   // its records, the slab's voxels, their occupancy words
    bool stopped = false;            // ev[1] is recorded (pass_stop: a pass that queues a read-back behind its timed part)
};

// `what` names the call in the message, `use` what the call does with the records and `multi` what it cannot do across ranks.
static int pass_open(vc_ctx *ctx, const char *what, const char *use, const char *multi, Pass &pass)
{
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "%s: no carve result", what);
    if (ctx->sb[ctx->cur].no_records)
        return fail(ctx, VC_ERR_ARG, "%s: the last carve ran with VC_FLAG_NO_RECORDS, there are no records to %s", what, use);
    if (ctx->comm && ctx->n_ranks > 1)
        return fail(ctx, VC_ERR_ARG, "%s: a communicator of %d ranks is attached (multi-GPU %s is not supported)", what, ctx->n_ranks, multi);
    if (ctx->z0 != 0 || ctx->z1 != ctx->nz)
        return fail(ctx, VC_ERR_ARG, "%s: the slab [%u,%u) is narrower than the grid's %u layers", what, ctx->z0, ctx->z1, ctx->nz);
    pass = Pass{&ctx->sb[ctx->cur], ctx->survivors, ctx->n_voxels(), (ctx->n_voxels() + 63) / 64, false};
    return VC_OK;
}

static int pass_begin(vc_ctx *ctx)
{
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(finish_gather(ctx));                  // (a compact gather of a one-rank communicator may still read the words)
    VC_HIP(ctx, ensure_pinned(ctx->h_res, 3));
    ctx->dist_ev_kind.clear();
    return VC_OK;
}

static int pass_start(vc_ctx *ctx, Pass &pass, PassWords words = kWordsIfRecords)
{
    // behind the step's record expansion (the second stream when overlap = 1; vc_carve_end has waited for it, this says so on the device)
    if (pass.S && pass.cur->n) VC_HIP(ctx, hipStreamWaitEvent(ctx->stream, pass.cur->e2, 0));
    VC_HIP(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    if (words == kWordsAlways || (words == kWordsIfRecords && pass.S)) VC_TRY(densify_words(ctx, *pass.cur));
    return VC_OK;
}

static int pass_stop(vc_ctx *ctx, Pass &pass)
{
    VC_HIP(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    pass.stopped = true;
    return VC_OK;
}

static int pass_end(vc_ctx *ctx, Pass &pass, float *ms)              // ms: where the elapsed time of ev[0] .. ev[1] goes (null: nowhere)
{
    if (!pass.stopped) VC_TRY(pass_stop(ctx, pass));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    dist_harvest(ctx);
    if (ms) VC_HIP(ctx, hipEventElapsedTime(ms, ctx->ev[0], ctx->ev[1]));
    return VC_OK;
}

// ---- occlusion-aware colouring of the current carve result (vc_visible.h; contract in include/voxcarve.h) ----
// The refusals vc_color_visible and vc_photo_carve share; `what` names the call in the message.
static int visible_refusals(vc_ctx *ctx, const char *what, uint32_t slot, float depth_tolerance, Pass &pass)
{
    VC_TRY(pass_open(ctx, what, "colour", "visibility", pass));
    if (!(depth_tolerance >= 0.0f)) return fail(ctx, VC_ERR_ARG, "%s: depth tolerance %g is negative or NaN", what, (double)depth_tolerance);
    if (slot >= ctx->slots.size() || !ctx->slots[slot].have_masks) return fail(ctx, VC_ERR_ARG, "%s: no frame set in slot %u", what, slot);
    const Slot &s = ctx->slots[slot];
    for (uint32_t c = 0; c < ctx->C; ++c)
        if (c >= s.have_frame.size() || !s.have_frame[c]) return fail(ctx, VC_ERR_ARG, "%s: camera %u has no frame in slot %u", what, c, slot);
    return VC_OK;
}

// The slot's images in the record layout, and the context's stream behind their preparation; then the pass starts (the occupancy
// words are made whole by enqueue_visible, behind the fill of the maps).
static int visible_start(vc_ctx *ctx, Slot &s, Pass &pass)
{
    if (!s.bits_valid) VC_TRY(ensure_prepared(ctx, s, false, nullptr));   // images uploaded after the carve: into the record layout
    if (s.prep_pending) { VC_HIP(ctx, hipStreamWaitEvent(ctx->stream, s.e_prep, 0)); s.prep_pending = false; }
    return pass_start(ctx, pass, kWordsLater);
}

// Queues items 1-4 of the colouring contract over records[0, S) of the current result on the context's stream: fill of the maps,
// surface list, splats.  rounds != null: records with rounds[s] != 0 are skipped (vc_photo_carve).  p is left filled for the
// kernel that follows (k_vis_color, k_photo_test), *lb with the grid those list kernels take.  No host synchronisation.
static int enqueue_visible(vc_ctx *ctx, Slot &s, StepBuf &cur, uint64_t *records, uint64_t S, float tol, const uint8_t *rounds,
                           VisParams &p, uint32_t &lb)
{
    const size_t HW = (size_t)ctx->H * ctx->W, nmap = HW * ctx->C;
    VC_TRY(ensure(ctx, ctx->visible.zmap, nmap));
    VC_TRY(ensure(ctx, ctx->visible.ctr, 4));
    VC_TRY(ensure(ctx, ctx->visible.mask, (size_t)S));
    VC_TRY(ensure(ctx, ctx->visible.list, (size_t)S));
    const dim3 block(kVisBlock);
    hipLaunchKernelGGL(k_vis_fill, dim3((uint32_t)((nmap + 4 * kVisBlock - 1) / (4 * kVisBlock))), block, 0, ctx->stream,
                       ctx->visible.zmap.ptr, (uint64_t)nmap, ctx->visible.ctr.ptr);
    VC_HIP(ctx, hipGetLastError());
    lb = 0;
    if (!S) return VC_OK;
    VC_TRY(densify_words(ctx, cur));
    VC_TRY(ensure(ctx, ctx->visible.queue, (size_t)kVisQueue));
    memset(&p, 0, sizeof p);
    p.xs = ctx->d_axes.ptr; p.ys = p.xs + ctx->nx; p.zs = p.ys + ctx->ny;
    p.words = cur.words.ptr;
    p.records = records;
    p.S = S;
    p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz; p.C = ctx->C; p.H = ctx->H; p.W = ctx->W;
    const double *b = ctx->bounds;                 // half the linspace step; 0 on an axis of one voxel
    p.hx = ctx->nx > 1 ? ((b[1] - b[0]) / (double)(ctx->nx - 1)) / 2.0 : 0.0;
    p.hy = ctx->ny > 1 ? ((b[3] - b[2]) / (double)(ctx->ny - 1)) / 2.0 : 0.0;
    p.hz = ctx->nz > 1 ? ((b[5] - b[4]) / (double)(ctx->nz - 1)) / 2.0 : 0.0;
    p.tol = tol;
    p.zmap = ctx->visible.zmap.ptr;
    p.frames = s.frames.ptr;
    p.vis = ctx->visible.mask.ptr;
    p.list = ctx->visible.list.ptr;
    p.ctr = ctx->visible.ctr.ptr;
    p.queue = ctx->visible.queue.ptr;
    p.big = (uint32_t)ctx->visible.big_rect;
    memcpy(p.cam, ctx->cams, sizeof(CamDev) * ctx->C);
    p.rounds = rounds;
    const uint64_t sblocks = (S + kVisBlock - 1) / kVisBlock;
    const dim3 sgrid((uint32_t)((S + kVisBlock * kVisSurfPer - 1) / (kVisBlock * kVisSurfPer)));
    if (rounds) hipLaunchKernelGGL(k_vis_surface<true>, sgrid, block, 0, ctx->stream, p);
    else hipLaunchKernelGGL(k_vis_surface<false>, sgrid, block, 0, ctx->stream, p);
    // the surface count stays on the device: the list kernels stride over it with a grid sized for all survivors, capped
    lb = (uint32_t)(sblocks < 2048 ? sblocks : 2048);
    if (ctx->visible.check) {
        hipLaunchKernelGGL(k_vis_splat<true>, dim3(lb, ctx->C), block, 0, ctx->stream, p);
        hipLaunchKernelGGL(k_vis_splat_big<true>, dim3(1024), block, 0, ctx->stream, p);
    } else {
        hipLaunchKernelGGL(k_vis_splat<false>, dim3(lb, ctx->C), block, 0, ctx->stream, p);
        hipLaunchKernelGGL(k_vis_splat_big<false>, dim3(1024), block, 0, ctx->stream, p);
    }
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// The whole colouring pass (items 1-5) over the current result's records; no host synchronisation.
static int enqueue_color_visible(vc_ctx *ctx, Slot &s, StepBuf &cur, float tol)
{
    VisParams p;
    uint32_t lb = 0;
    VC_TRY(enqueue_visible(ctx, s, cur, cur.records.ptr, ctx->survivors, tol, nullptr, p, lb));
    if (lb) {
        hipLaunchKernelGGL(k_vis_color, dim3(lb), dim3(kVisBlock), 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
    }
    return VC_OK;
}

int vc_color_visible(vc_ctx *ctx, uint32_t slot, float depth_tolerance, uint32_t flags)
{
    if (!ctx) return VC_ERR_ARG;
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_color_visible: flags must be 0 (got %u)", flags);
    Pass pass;
    VC_TRY(visible_refusals(ctx, "vc_color_visible", slot, depth_tolerance, pass));
    Slot &s = ctx->slots[slot];
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->visible.stamp = kNever;
    VC_TRY(visible_start(ctx, s, pass));
    VC_TRY(enqueue_color_visible(ctx, s, cur, depth_tolerance));
    VC_TRY(pass_end(ctx, pass, &ctx->tm.visible_ms));
    ctx->visible.stamp = ctx->result_gen;
    return VC_OK;
}

// ---- photo-consistency carving of the current carve result (vc_photo.h; contract in include/voxcarve.h) ----
int vc_photo_carve(vc_ctx *ctx, uint32_t slot, float depth_tolerance, uint32_t var_threshold, uint32_t min_views,
                   uint32_t max_rounds, uint32_t flags, vc_photo_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_photo_carve: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_photo_carve: flags must be 0 (got %u)", flags);
    Pass pass;
    VC_TRY(visible_refusals(ctx, "vc_photo_carve", slot, depth_tolerance, pass));
    if (min_views < 2 || min_views > ctx->C)
        return fail(ctx, VC_ERR_ARG, "vc_photo_carve: min_views %u not in [2, %u] (2 .. the number of cameras)", min_views, ctx->C);
    if (max_rounds < 1 || max_rounds > kPhotoMaxRounds)
        return fail(ctx, VC_ERR_ARG, "vc_photo_carve: max_rounds %u not in [1, %u]", max_rounds, kPhotoMaxRounds);
    Slot &s = ctx->slots[slot];
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    result_changed(ctx);
    const uint64_t S0 = pass.S;
    VC_TRY(ensure(ctx, ctx->photo.rounds, (size_t)S0));
    VC_TRY(ensure(ctx, ctx->photo.removed, kPhotoMaxRounds + 1));
    VC_TRY(visible_start(ctx, s, pass));
    if (S0) VC_HIP(ctx, hipMemsetAsync(ctx->photo.rounds.ptr, 0, (size_t)S0, ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(ctx->photo.removed.ptr, 0, (kPhotoMaxRounds + 1) * sizeof(uint32_t), ctx->stream));
    PhotoParams q;
    memset(&q, 0, sizeof q);
    q.rounds = ctx->photo.rounds.ptr;
    q.words = cur.words.ptr;
    q.thr = var_threshold;
    q.min_views = min_views;
    uint64_t left = S0;
    uint32_t r = 0;
    bool converged = false;
    while (r < max_rounds) {
        ++r;
        VisParams p;
        uint32_t lb = 0;
        VC_TRY(enqueue_visible(ctx, s, cur, cur.records.ptr, S0, depth_tolerance, q.rounds, p, lb));
        q.removed = ctx->photo.removed.ptr + r;
        q.round = r;
        if (lb) {
            hipLaunchKernelGGL(k_photo_test, dim3(lb), dim3(kVisBlock), 0, ctx->stream, p, q);
            VC_HIP(ctx, hipGetLastError());
        }
        // 4 bytes back per round: the loop ends on the first round without removals
        ctx->h_res[0] = 0;
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res, q.removed, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t gone = (uint32_t)ctx->h_res[0];
        if (gone > left) return fail(ctx, VC_ERR_HIP, "vc_photo_carve: round %u removed %u of %llu survivors", r, gone, (unsigned long long)left);
        if (gone == 0) { converged = true; break; }
        left -= gone;
    }
    if (left != S0) {
        VC_TRY(compact_records(ctx, cur, PhotoKept{q.rounds, cur.records.ptr, nullptr}, S0, ctx->h_res + 1));
        ctx->survivors = cur.survivors = left;
    }
    VC_TRY(enqueue_color_visible(ctx, s, cur, depth_tolerance));   // the colouring of F: its maps, masks and colours
    VC_TRY(pass_end(ctx, pass, &stats->photo_ms));
    if (left != S0 && ctx->h_res[1] != left)
        return fail(ctx, VC_ERR_HIP, "vc_photo_carve: the compaction kept %llu records, the rounds left %llu",
                    (unsigned long long)ctx->h_res[1], (unsigned long long)left);
    stats->rounds = r;
    stats->converged = converged ? 1u : 0u;
    stats->survivors_before = S0;
    stats->survivors_after = left;
    ctx->visible.stamp = ctx->result_gen;
    ctx->photo.stamp = ctx->result_gen;
    ctx->photo.n = S0;
    return VC_OK;
}

int vc_fetch_photo_rounds(vc_ctx *ctx, uint8_t *rounds)
{
    if (!ctx || !rounds) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->photo.stamp)) return fail(ctx, VC_ERR_ARG, "no photo rounds: call vc_photo_carve on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->photo.n) VC_HIP(ctx, hipMemcpy(rounds, ctx->photo.rounds.ptr, (size_t)ctx->photo.n, hipMemcpyDeviceToHost));
    return VC_OK;
}

// ---- connected components of the current carve result (vc_components.h; contract in include/voxcarve.h) ----
int vc_hull_components(vc_ctx *ctx, uint32_t connectivity, uint64_t min_voxels, uint32_t keep_largest, uint32_t flags,
                       vc_component_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_components: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_components: flags must be 0 (got %u)", flags);
    if (connectivity != 6 && connectivity != 18 && connectivity != 26)
        return fail(ctx, VC_ERR_ARG, "vc_hull_components: connectivity %u, expected 6, 18 or 26", connectivity);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_components", "label", "labelling", pass));
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    result_changed(ctx);
    const uint64_t S0 = pass.S, nwords = pass.nwords;
    VC_TRY(pass_start(ctx, pass));
    uint32_t K = 0;
    uint64_t kept_records = 0;
    if (S0) {
        const uint32_t wgroups = word_groups(nwords);
        const uint32_t rgroups = (uint32_t)((S0 + kCompactGroup - 1) / kCompactGroup);
        VC_TRY(ensure(ctx, ctx->d_rscan, wgroups > rgroups ? wgroups : rgroups));
        VC_TRY(ensure(ctx, ctx->d_woff, (size_t)nwords));
        VC_TRY(ensure(ctx, ctx->components.parent, (size_t)S0));
        VC_TRY(ensure(ctx, ctx->components.label, (size_t)S0));
        VC_TRY(ensure(ctx, ctx->components.cid, (size_t)S0));
        VC_TRY(ensure(ctx, ctx->components.roots, (size_t)S0));        // (K <= S0: sized before the count is known)
        VC_TRY(ensure(ctx, ctx->components.misc, 2));
        VC_TRY(ensure(ctx, ctx->components.thr, 1));
        // 1 survivors before each word
        const dim3 block(kCcBlock);
        VC_TRY(word_offsets(ctx, cur, nwords, ctx->d_woff, ctx->h_res + 1));
        CcParams p;
        memset(&p, 0, sizeof p);
        p.records = cur.records.ptr;
        p.words = cur.words.ptr;
        p.woff = ctx->d_woff.ptr;
        p.parent = ctx->components.parent.ptr;
        p.label = ctx->components.label.ptr;
        p.cid = ctx->components.cid.ptr;
        p.S = S0;
        p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz;
        // 2-4 runs, unions across runs, compression
        const dim3 sgrid((uint32_t)((S0 + kCcBlock - 1) / kCcBlock));
        hipLaunchKernelGGL(k_cc_init, sgrid, block, 0, ctx->stream, p);
        if (connectivity == 6) hipLaunchKernelGGL(k_cc_union<6>, sgrid, block, 0, ctx->stream, p);
        else if (connectivity == 18) hipLaunchKernelGGL(k_cc_union<18>, sgrid, block, 0, ctx->stream, p);
        else hipLaunchKernelGGL(k_cc_union<26>, sgrid, block, 0, ctx->stream, p);
        hipLaunchKernelGGL(k_cc_compress, sgrid, block, 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
        // 6 the roots, compacted stably: the component list in ascending label
        VC_TRY(compact(ctx, CcRoots{p.parent, ctx->components.roots.ptr, p.cid}, S0, ctx->h_res + 0));
        // the one read-back before the end: the number of components sizes their arrays
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const uint64_t K64 = ctx->h_res[0];
        if (K64 == 0 || K64 > S0)
            return fail(ctx, VC_ERR_HIP, "vc_hull_components: %llu components among %llu survivors", (unsigned long long)K64,
                        (unsigned long long)S0);
        K = (uint32_t)K64;
        VC_TRY(ensure(ctx, ctx->components.size, K));
        VC_TRY(ensure(ctx, ctx->components.box, (size_t)K * 6));
        VC_TRY(ensure(ctx, ctx->components.kept, K));
        VC_TRY(ensure(ctx, ctx->components.comp, (size_t)K * kCcCompWords));
        p.roots = ctx->components.roots.ptr;
        p.size = ctx->components.size.ptr;
        p.box = ctx->components.box.ptr;
        p.kept = ctx->components.kept.ptr;
        VC_HIP(ctx, hipMemsetAsync(ctx->components.misc.ptr, 0, 2 * sizeof(uint32_t), ctx->stream));
        // 5 sizes and boxes; 7 the keep rule
        hipLaunchKernelGGL(k_cc_clear, dim3((K + kCcBlock - 1) / kCcBlock), block, 0, ctx->stream, p, K);
        hipLaunchKernelGGL(k_cc_stats, dim3(rgroups), block, 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
        const uint32_t want = keep_largest < K ? keep_largest : 0u;             // keep_largest >= K: no component is out of rank
        hipLaunchKernelGGL(k_cc_select, dim3(1), dim3(kCcSelectBlock), 0, ctx->stream, (const uint32_t *)p.size, K, want, ctx->components.thr.ptr);
        hipLaunchKernelGGL(k_cc_mark, dim3((K + kCcBlock - 1) / kCcBlock), block, 0, ctx->stream, p, K, min_voxels,
                           (const uint64_t *)ctx->components.thr.ptr, ctx->components.kept.ptr, ctx->components.comp.ptr, ctx->components.misc.ptr);
        VC_HIP(ctx, hipGetLastError());
        // 8 the kept records, stably, become the step's (the dropped ones leave the words)
        VC_TRY(compact_records(ctx, cur, CcKept{p.parent, p.cid, p.kept, p.records, p.words, nullptr}, S0, ctx->h_res + 1));
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res + 2, ctx->components.misc.ptr, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    VC_TRY(pass_end(ctx, pass, &stats->components_ms));
    uint32_t kept_components = 0, largest = 0;
    if (S0) {
        kept_records = ctx->h_res[1];
        kept_components = (uint32_t)ctx->h_res[2];
        largest = (uint32_t)(ctx->h_res[2] >> 32);
        ctx->survivors = cur.survivors = kept_records;
        if (kept_records > S0 || kept_components > K)
            return fail(ctx, VC_ERR_HIP, "vc_hull_components: kept %llu of %llu records, %u of %u components", (unsigned long long)kept_records,
                        (unsigned long long)S0, kept_components, K);
    }
    stats->components = K;
    stats->components_kept = kept_components;
    stats->survivors_before = S0;
    stats->survivors_after = kept_records;
    stats->largest = largest;
    ctx->components.stamp = ctx->result_gen;
    ctx->components.n = S0;
    ctx->components.k = K;
    return VC_OK;
}

int vc_fetch_component_labels(vc_ctx *ctx, uint32_t *labels)
{
    if (!ctx || !labels) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->components.stamp)) return fail(ctx, VC_ERR_ARG, "no component labels: call vc_hull_components on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->components.n) VC_HIP(ctx, hipMemcpy(labels, ctx->components.label.ptr, (size_t)ctx->components.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_components(vc_ctx *ctx, vc_component_t *out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->components.stamp)) return fail(ctx, VC_ERR_ARG, "no components: call vc_hull_components on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(vc_component_t) == kCcCompWords * sizeof(uint32_t), "vc_component_t is the device's entry");
    if (ctx->components.k) VC_HIP(ctx, hipMemcpy(out, ctx->components.comp.ptr, (size_t)ctx->components.k * sizeof(vc_component_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

// ---- distance field of the current carve result; erosion and opening (vc_distance.h; contract in include/voxcarve.h) ----
// Item 2 of the contract: the steps in micrometres, q = x, y, z (the first `axes` of them: vc_hull_clusters takes x and y).
static int dist_metric(vc_ctx *ctx, const char *what, uint64_t *q, int axes = 3)
{
    const uint32_t n[3] = {ctx->nx, ctx->ny, ctx->nz};
    for (int a = 0; a < axes; ++a) {
        if (n[a] < 2) return fail(ctx, VC_ERR_ARG, "%s: axis %c has %u cells, a step needs 2", what, "xyz"[a], n[a]);
        const double s = (ctx->bounds[2 * a + 1] - ctx->bounds[2 * a]) / (double)(n[a] - 1);
        const long long v = llrint(s * 1000.0);
        if (!(s * 1000.0 >= 0.5) || !(s * 1000.0 < 2097152.0) || v < 1 || v > (1ll << 20))
            return fail(ctx, VC_ERR_ARG, "%s: the step of axis %c is %g mm, outside 1 um .. 2^20 um", what, "xyz"[a], s);
        if ((uint64_t)(n[a] + 1) * (uint64_t)v > (1ull << 30))
            return fail(ctx, VC_ERR_ARG, "%s: axis %c spans (%u + 1) x %lld um, above 2^30 um", what, "xyz"[a], n[a], v);
        if (n[a] + 2 > kDistMaxLine)
            return fail(ctx, VC_ERR_ARG, "%s: axis %c has %u cells, lines hold at most %u", what, "xyz"[a], n[a], kDistMaxLine - 2);
        q[a] = (uint64_t)v;
    }
    return VC_OK;
}

static uint64_t dist_cells(const DistBox &bx) { return (uint64_t)bx.b[0] * bx.b[1] * bx.b[2]; }

// Sizes the fields of a transform over bx: f, the other field of the envelope passes and the stacks.
static int dist_ensure(vc_ctx *ctx, DevBuf<uint64_t> &f, const DistBox &bx)
{
    const uint64_t cells = dist_cells(bx);
    VC_TRY(ensure(ctx, f, (size_t)cells));
    VC_TRY(ensure(ctx, ctx->distance.tmp, (size_t)cells));
    VC_TRY(ensure(ctx, ctx->distance.st, (size_t)cells));
    return VC_OK;
}

// Queues one transform over bx on the context's stream: f = squared distance to the nearest site of `mode` (kDistSiteAbove: the
// cells of f itself above r2).  Buffers sized by dist_ensure.
static int dist_transform(vc_ctx *ctx, const DistBox &bx, int mode, const uint64_t *words, uint64_t *f, uint64_t r2, const uint64_t q[3])
{
    const uint64_t plane = (uint64_t)bx.b[0] * bx.b[1], ylines = (uint64_t)bx.b[0] * bx.b[2], xlines = (uint64_t)bx.b[1] * bx.b[2];
    const dim3 block(kDistBlock), ygrid((uint32_t)((ylines + kDistBlock / 64 - 1) / (kDistBlock / 64)));
    if (mode == kDistSiteOff) VC_DLAUNCH(VC_K_DIST_Y, k_dist_y<kDistSiteOff>, ygrid, block, bx, words, f, r2, q[1]);
    else if (mode == kDistSiteOn) VC_DLAUNCH(VC_K_DIST_Y, k_dist_y<kDistSiteOn>, ygrid, block, bx, words, f, r2, q[1]);
    else VC_DLAUNCH(VC_K_DIST_Y, k_dist_y<kDistSiteAbove>, ygrid, block, bx, words, f, r2, q[1]);
    // along x: line (lz, ly) from f into the other field; along z: line (lx, ly) back into f
    VC_DLAUNCH(VC_K_DIST_ENV, k_dist_env, dim3((uint32_t)((xlines + kDistBlock - 1) / kDistBlock)), block, (const uint64_t *)f,
               ctx->distance.tmp.ptr, ctx->distance.st.ptr, xlines, (uint64_t)bx.b[1], plane, (uint64_t)bx.b[1], bx.b[0], q[0] * q[0]);
    VC_DLAUNCH(VC_K_DIST_ENV, k_dist_env, dim3((uint32_t)((plane + kDistBlock - 1) / kDistBlock)), block,
               (const uint64_t *)ctx->distance.tmp.ptr, f, ctx->distance.st.ptr, plane, plane, (uint64_t)0, plane, bx.b[2], q[2] * q[2]);
    VC_HIP(ctx, hipGetLastError());
    ctx->distance.work[0] += dist_cells(bx);
    ctx->distance.work[1] += ylines + xlines + plane;
    return VC_OK;
}

// Queues the records' values of the box field f: d_dist_rec[s], and acc[0] = their maximum, acc[1] = how many lie above r2.
static int dist_records(vc_ctx *ctx, StepBuf &cur, const DistBox &bx, const uint64_t *f, uint64_t S, uint64_t r2, unsigned long long *acc)
{
    VC_HIP(ctx, hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), ctx->stream));
    VC_DLAUNCH(VC_K_DIST_RECORDS, k_dist_records, dim3((uint32_t)((S + kDistGroup - 1) / kDistGroup)), dim3(kDistBlock), bx,
               (const uint64_t *)cur.records.ptr, S, f, r2, ctx->distance.rec.ptr, acc);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// The inclusive index box of the current result's S > 0 records (one read-back): hb[0..2] = min ix, iy, iz, hb[3..5] = max,
// hb = the pinned scalars.
static int dist_survivor_box(vc_ctx *ctx, StepBuf &cur, uint64_t S, uint32_t *&hb)
{
    VC_TRY(ensure(ctx, ctx->distance.d_box, 6));
    hb = reinterpret_cast<uint32_t *>(ctx->h_res.ptr);
    hb[0] = hb[1] = hb[2] = 0xffffffffu; hb[3] = hb[4] = hb[5] = 0;
    VC_HIP(ctx, hipMemcpyAsync(ctx->distance.d_box.ptr, hb, 6 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VC_DLAUNCH(VC_K_DIST_BOX, k_dist_box, dim3((uint32_t)((S + kDistGroup - 1) / kDistGroup)), dim3(kDistBlock),
               (const uint64_t *)cur.records.ptr, S, ctx->nx, ctx->ny, ctx->distance.d_box.ptr);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(hb, ctx->distance.d_box.ptr, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n[3] = {ctx->nx, ctx->ny, ctx->nz};
    for (int a = 0; a < 3; ++a)
        if (hb[a] > hb[3 + a] || hb[3 + a] >= n[a])
            return fail(ctx, VC_ERR_HIP, "the survivors' box [%u, %u] on axis %c of %u cells", hb[a], hb[3 + a], "xyz"[a], n[a]);
    return VC_OK;
}

// The inside field of the current result's S > 0 records: their index box, grown by a cell per side and, with the border open,
// clipped to the grid; the transform into d_dist_in over that box; the records' values and acc[0..1] against r2.
static int dist_inside(vc_ctx *ctx, StepBuf &cur, uint32_t flags, uint64_t S, uint64_t r2, const uint64_t q[3], DistBox &bx)
{
    VC_TRY(ensure(ctx, ctx->distance.acc, 4));
    VC_TRY(ensure(ctx, ctx->distance.rec, (size_t)S));
    uint32_t *hb = nullptr;
    VC_TRY(dist_survivor_box(ctx, cur, S, hb));
    const uint32_t n[3] = {ctx->nx, ctx->ny, ctx->nz};
    memset(&bx, 0, sizeof bx);
    bx.nx = ctx->nx; bx.ny = ctx->ny; bx.nz = ctx->nz;
    for (int a = 0; a < 3; ++a) {
        int32_t lo = (int32_t)hb[a] - 1, hi = (int32_t)hb[3 + a] + 1;
        if (!(flags & VC_DIST_BORDER_OFF)) { lo = lo < 0 ? 0 : lo; hi = hi >= (int32_t)n[a] ? (int32_t)n[a] - 1 : hi; }
        bx.o[a] = lo;
        bx.b[a] = (uint32_t)(hi - lo + 1);
    }
    VC_TRY(dist_ensure(ctx, ctx->distance.in, bx));
    VC_TRY(dist_transform(ctx, bx, kDistSiteOff, cur.words.ptr, ctx->distance.in.ptr, 0, q));
    VC_TRY(dist_records(ctx, cur, bx, ctx->distance.in.ptr, S, r2, ctx->distance.acc.ptr));
    return VC_OK;
}

int vc_hull_distance(vc_ctx *ctx, uint32_t flags, vc_distance_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_distance: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags & ~(VC_DIST_BORDER_OFF | VC_DIST_OUTSIDE))
        return fail(ctx, VC_ERR_ARG, "vc_hull_distance: unknown flags %u (VC_DIST_BORDER_OFF | VC_DIST_OUTSIDE)", flags);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_distance", "measure", "distance transforms", pass));
    uint64_t q[3];
    VC_TRY(dist_metric(ctx, "vc_hull_distance", q));
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->distance.stamp = kNever;
    const uint64_t S = pass.S, n = pass.n;
    const bool outside = (flags & VC_DIST_OUTSIDE) != 0;
    VC_TRY(pass_start(ctx, pass));
    DistBox bx;
    memset(&bx, 0, sizeof bx);
    if (S) {
        VC_TRY(dist_inside(ctx, cur, flags, S, 0, q, bx));
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res, ctx->distance.acc.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (outside) {
        if (S) {
            DistBox all;
            memset(&all, 0, sizeof all);
            all.nx = all.b[0] = ctx->nx; all.ny = all.b[1] = ctx->ny; all.nz = all.b[2] = ctx->nz;
            VC_TRY(dist_ensure(ctx, ctx->distance.out, all));
            VC_TRY(dist_transform(ctx, all, kDistSiteOn, cur.words.ptr, ctx->distance.out.ptr, 0, q));
        } else {
            VC_TRY(ensure(ctx, ctx->distance.out, (size_t)n));
            VC_HIP(ctx, hipMemsetAsync(ctx->distance.out.ptr, 0xff, (size_t)n * sizeof(uint64_t), ctx->stream));
        }
    }
    VC_TRY(pass_end(ctx, pass, &stats->distance_ms));
    stats->survivors = S;
    stats->sites_inside_box = S ? dist_cells(bx) - S : 0;
    stats->max_d2 = S ? ctx->h_res[0] : 0;
    for (int a = 0; a < 3; ++a) stats->q[a] = q[a];
    ctx->distance.stamp = ctx->result_gen;
    ctx->distance.outside = outside;
    ctx->distance.n = S;
    ctx->distance.box = bx;
    return VC_OK;
}

int vc_fetch_record_distance(vc_ctx *ctx, uint64_t *d2)
{
    if (!ctx || !d2) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->distance.stamp)) return fail(ctx, VC_ERR_ARG, "no distance field: call vc_hull_distance on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->distance.n) VC_HIP(ctx, hipMemcpy(d2, ctx->distance.rec.ptr, (size_t)ctx->distance.n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_distance(vc_ctx *ctx, uint32_t which, uint64_t *d2)
{
    if (!ctx || !d2) return VC_ERR_ARG;
    if (which > 1) return fail(ctx, VC_ERR_ARG, "vc_fetch_distance: which = %u, expected 0 (inside) or 1 (outside)", which);
    if (!ctx->carved || !ctx->current(ctx->distance.stamp)) return fail(ctx, VC_ERR_ARG, "no distance field: call vc_hull_distance on the current carve result");
    if (which == 1 && !ctx->distance.outside)
        return fail(ctx, VC_ERR_ARG, "no outside field: the last vc_hull_distance ran without VC_DIST_OUTSIDE");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = ctx->n_voxels();
    if (which == 1) {
        if (n) VC_HIP(ctx, hipMemcpy(d2, ctx->distance.out.ptr, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return VC_OK;
    }
    memset(d2, 0, (size_t)n * sizeof(uint64_t));                 // zero off the box: every voxel there is OFF
    if (!ctx->distance.n) return VC_OK;
    const DistBox &bx = ctx->distance.box;
    std::vector<uint64_t> h((size_t)dist_cells(bx));
    VC_HIP(ctx, hipMemcpy(h.data(), ctx->distance.in.ptr, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    // the rows of the box that lie in the grid, cut to the grid along y
    const int32_t y0 = bx.o[1] < 0 ? 0 : bx.o[1], y1 = std::min<int32_t>(bx.o[1] + (int32_t)bx.b[1], (int32_t)bx.ny);
    for (uint32_t lz = 0; lz < bx.b[2]; ++lz) {
        const int32_t gz = bx.o[2] + (int32_t)lz;
        if (gz < 0 || gz >= (int32_t)bx.nz) continue;
        for (uint32_t lx = 0; lx < bx.b[0]; ++lx) {
            const int32_t gx = bx.o[0] + (int32_t)lx;
            if (gx < 0 || gx >= (int32_t)bx.nx) continue;
            const uint64_t *src = h.data() + ((size_t)lz * bx.b[0] + lx) * bx.b[1] + (size_t)(y0 - bx.o[1]);
            memcpy(d2 + ((size_t)gz * bx.nx + (size_t)gx) * bx.ny + (size_t)y0, src, (size_t)(y1 - y0) * sizeof(uint64_t));
        }
    }
    return VC_OK;
}

int vc_hull_morphology(vc_ctx *ctx, uint32_t op, uint64_t r2, uint32_t flags, vc_morph_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_morphology: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (op != VC_MORPH_ERODE && op != VC_MORPH_OPEN)
        return fail(ctx, VC_ERR_ARG, "vc_hull_morphology: unknown op %u (VC_MORPH_ERODE, VC_MORPH_OPEN)", op);
    if (flags & ~VC_DIST_BORDER_OFF) return fail(ctx, VC_ERR_ARG, "vc_hull_morphology: unknown flags %u (VC_DIST_BORDER_OFF)", flags);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_morphology", "keep", "morphology", pass));
    uint64_t q[3];
    VC_TRY(dist_metric(ctx, "vc_hull_morphology", q));
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    const uint64_t S0 = pass.S;
    if (S0) {                                    // every buffer of the hand-over before anything is queued: a failure leaves the result
        VC_TRY(ensure(ctx, ctx->d_rec_spare, cur.records.cap));
        VC_TRY(ensure(ctx, ctx->d_rscan, (uint32_t)((S0 + kCompactGroup - 1) / kCompactGroup)));
    }
    VC_TRY(pass_start(ctx, pass));
    if (S0) {
        DistBox bx;
        VC_TRY(dist_inside(ctx, cur, flags, S0, r2, q, bx));     // 5: d_dist_rec = D_in, acc = [max D_in, |E|]
        if (op == VC_MORPH_OPEN) {                               // 6: the same transform with sites = E, over the same box
            VC_TRY(dist_transform(ctx, bx, kDistSiteAbove, cur.words.ptr, ctx->distance.in.ptr, r2, q));
            VC_TRY(dist_records(ctx, cur, bx, ctx->distance.in.ptr, S0, r2, ctx->distance.acc.ptr + 2));
        }
        // the result changes from here on
        result_changed(ctx);
        VC_TRY(compact_records(ctx, cur, DistKept{ctx->distance.rec.ptr, r2, op == VC_MORPH_OPEN ? 1u : 0u, cur.records.ptr, cur.words.ptr, nullptr},
                               S0, ctx->h_res + 1));
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res + 0, ctx->distance.acc.ptr + 0, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res + 2, ctx->distance.acc.ptr + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    result_changed(ctx);
    VC_TRY(pass_end(ctx, pass, &stats->morph_ms));
    uint64_t kept = 0;
    if (S0) {
        kept = ctx->h_res[1];
        if (kept > S0) return fail(ctx, VC_ERR_HIP, "vc_hull_morphology: kept %llu of %llu records", (unsigned long long)kept, (unsigned long long)S0);
        ctx->survivors = cur.survivors = kept;
        stats->max_d2 = ctx->h_res[0];
        stats->eroded = ctx->h_res[2];
    }
    stats->survivors_before = S0;
    stats->survivors_after = kept;
    for (int a = 0; a < 3; ++a) stats->q[a] = q[a];
    return VC_OK;
}

// ---- dilation and closing of the current carve result (vc_grow.h; contract in include/voxcarve.h) ----
// floor(sqrt(v)) exactly
static uint64_t isqrt_u64(uint64_t v)
{
    uint64_t r = (uint64_t)std::sqrt((long double)v);
    while (r > 0xffffffffull || r * r > v) --r;
    while (r < 0xffffffffull && (r + 1) * (r + 1) <= v) ++r;
    return r;
}

int vc_hull_grow(vc_ctx *ctx, uint32_t op, uint64_t r2, uint32_t flags, vc_grow_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_grow: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (op != VC_GROW_DILATE && op != VC_GROW_CLOSE)
        return fail(ctx, VC_ERR_ARG, "vc_hull_grow: unknown op %u (VC_GROW_DILATE, VC_GROW_CLOSE)", op);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_grow: flags must be 0 (got %u)", flags);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_grow", "merge the added voxels into", "morphology", pass));
    uint64_t q[3];
    VC_TRY(dist_metric(ctx, "vc_hull_grow", q));
    StepBuf &cur = *pass.cur;
    VC_TRY(merge_refuse_slot(ctx, "vc_hull_grow", cur));
    const uint64_t n = pass.n, nwords = pass.nwords;
    VC_TRY(merge_refuse_index(ctx, "vc_hull_grow", n));
    VC_TRY(pass_begin(ctx));
    const uint64_t S0 = pass.S;
    VC_TRY(pass_start(ctx, pass));
    uint64_t S1 = S0, added = 0, dilated = 0;
    DistBox bx;
    memset(&bx, 0, sizeof bx);
    if (S0) {
        // the survivors' index box, grown per axis by g_a + 1 cells and clipped to the grid: Dl lies inside the g-grown box, and the
        // extra layer (where no grid face cuts it off) is outside Dl, which makes the second transform over the box exact
        uint32_t *hb = nullptr;
        VC_TRY(dist_survivor_box(ctx, cur, S0, hb));
        const uint32_t dims[3] = {ctx->nx, ctx->ny, ctx->nz};
        const uint64_t root = isqrt_u64(r2);
        bx.nx = ctx->nx; bx.ny = ctx->ny; bx.nz = ctx->nz;
        for (int a = 0; a < 3; ++a) {
            const int64_t g = (int64_t)(root / q[a]) + 1;
            const int64_t lo = std::max<int64_t>((int64_t)hb[a] - g, 0), hi = std::min<int64_t>((int64_t)hb[3 + a] + g, (int64_t)dims[a] - 1);
            bx.o[a] = (int32_t)lo;
            bx.b[a] = (uint32_t)(hi - lo + 1);
        }
        // the occupancy words the box spans: the added bits are collected in a zeroed copy of that range
        const uint64_t i_lo = ((uint64_t)bx.o[2] * ctx->nx + (uint32_t)bx.o[0]) * ctx->ny + (uint32_t)bx.o[1];
        const uint64_t i_hi = ((uint64_t)(bx.o[2] + (int32_t)bx.b[2] - 1) * ctx->nx + (uint32_t)(bx.o[0] + (int32_t)bx.b[0] - 1)) * ctx->ny +
                              (uint32_t)(bx.o[1] + (int32_t)bx.b[1] - 1);
        const uint64_t w0 = i_lo >> 6, nrange = (i_hi >> 6) - w0 + 1;
        ctx->distance.stamp = kNever;            // the field's buffer is the transforms' from here on, whether the call succeeds or not
        VC_TRY(dist_ensure(ctx, ctx->distance.in, bx));
        VC_TRY(ensure(ctx, ctx->grow.addw, (size_t)nrange));
        VC_TRY(ensure(ctx, ctx->grow.ctr, 2));
        uint64_t *f = ctx->distance.in.ptr;
        const uint64_t ylines = (uint64_t)bx.b[0] * bx.b[2];
        const dim3 block(kDistBlock), mgrid((uint32_t)((ylines + (kDistBlock / 64) * kGrowLines - 1) / ((kDistBlock / 64) * kGrowLines)));
        VC_HIP(ctx, hipMemsetAsync(ctx->grow.ctr.ptr, 0, 2 * sizeof(unsigned long long), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(ctx->grow.addw.ptr, 0, (size_t)nrange * sizeof(unsigned long long), ctx->stream));
        // 1: D_out over the box; 2: for the closing |Dl|, then the same transform with sites = the box's cells outside Dl
        VC_TRY(dist_transform(ctx, bx, kDistSiteOn, cur.words.ptr, f, 0, q));
        if (op == VC_GROW_CLOSE) {
            VC_DLAUNCH(VC_K_GROW_MARK, k_grow_mark<kGrowCount>, mgrid, block, bx, (const uint64_t *)f, r2, (const uint64_t *)cur.words.ptr, nwords,
                       ctx->grow.addw.ptr, w0, nrange, ctx->grow.ctr.ptr + 1);
            VC_TRY(dist_transform(ctx, bx, kDistSiteAbove, cur.words.ptr, f, r2, q));
            VC_DLAUNCH(VC_K_GROW_MARK, k_grow_mark<kGrowClose>, mgrid, block, bx, (const uint64_t *)f, r2, (const uint64_t *)cur.words.ptr, nwords,
                       ctx->grow.addw.ptr, w0, nrange, ctx->grow.ctr.ptr + 0);
        } else {
            VC_DLAUNCH(VC_K_GROW_MARK, k_grow_mark<kGrowDilate>, mgrid, block, bx, (const uint64_t *)f, r2, (const uint64_t *)cur.words.ptr, nwords,
                       ctx->grow.addw.ptr, w0, nrange, ctx->grow.ctr.ptr + 0);
        }
        VC_HIP(ctx, hipGetLastError());
        // the read-back in the middle: the added voxels size the records
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res, ctx->grow.ctr.ptr, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        added = ctx->h_res[0];
        S1 = S0 + added;
        dilated = op == VC_GROW_CLOSE ? ctx->h_res[1] : S1;
        if (S1 > n || dilated < S1 || dilated > n)
            return fail(ctx, VC_ERR_HIP, "vc_hull_grow: %llu added to %llu survivors, %llu dilated, in a grid of %llu voxels", (unsigned long long)added,
                        (unsigned long long)S0, (unsigned long long)dilated, (unsigned long long)n);
        // every buffer of the hand-over before anything changes: a failure leaves the result
        ctx->grow.stamp = kNever;                // (the added bytes of an earlier call go with their buffer)
        VC_TRY(ensure(ctx, ctx->grow.added, (size_t)S1));
        VC_HIP(ctx, hipMemsetAsync(ctx->grow.added.ptr, 0, (size_t)S1, ctx->stream));   // (the pass's own bytes, stamp dropped above)
        if (added) {
            MergeParams p;
            VC_TRY(merge_sized(ctx, cur, nwords, S1, true, ctx->grow.added.ptr, p));
            // the result changes from here on
            result_changed(ctx);
            const dim3 gblock(kGrowBlock), rgrid((uint32_t)((nrange + kGrowBlock - 1) / kGrowBlock));
            const unsigned long long *addw = ctx->grow.addw.ptr;
            VC_DLAUNCH(VC_K_GROW_RANK, k_grow_apply, rgrid, gblock, cur.words.ptr, nwords, addw, w0, nrange);
            VC_TRY(merge_ranked(ctx, cur, p, nwords, S0, true, VC_K_GROW_RANK, VC_K_GROW_MERGE));
            VC_DLAUNCH(VC_K_GROW_MERGE, k_grow_new, rgrid, gblock, p, addw, w0, nrange, nwords);   // a fresh record for every added voxel
            VC_HIP(ctx, hipGetLastError());
            VC_TRY(records_handed_over(ctx, cur, word_groups(nwords)));
        }
    }
    // a call that adds nothing (r2 = 0, a second closing, the empty hull) leaves the result as it is, and with it the visibility,
    // the photo rounds and the component labels; the stored distance field went with its buffer above
    ctx->grow.stamp = kNever;
    VC_TRY(pass_end(ctx, pass, &stats->grow_ms));
    if (added) {
        ctx->survivors = cur.survivors = S1;
        VC_TRY(merge_counted(ctx, "vc_hull_grow", S1, "records were merged"));
    }
    stats->survivors_before = S0;
    stats->dilated = dilated;
    stats->survivors_after = S1;
    stats->added = added;
    stats->box_cells = S0 ? dist_cells(bx) : 0;
    for (int a = 0; a < 3; ++a) stats->q[a] = q[a];
    ctx->grow.stamp = ctx->result_gen;
    ctx->grow.n = S1;
    return VC_OK;
}

int vc_fetch_grown(vc_ctx *ctx, uint8_t *added)
{
    if (!ctx || !added) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->grow.stamp)) return fail(ctx, VC_ERR_ARG, "no added flags: call vc_hull_grow on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->grow.n) VC_HIP(ctx, hipMemcpy(added, ctx->grow.added.ptr, (size_t)ctx->grow.n, hipMemcpyDeviceToHost));
    return VC_OK;
}

// ---- the vote over the last frames' hulls (vc_temporal.h; contract in include/voxcarve.h) ----
int vc_hull_temporal(vc_ctx *ctx, uint32_t window, uint32_t keep_on, uint32_t keep_off, uint32_t flags, vc_temporal_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_temporal: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_temporal: flags must be 0 (got %u)", flags);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_temporal", "vote on", "temporal voting", pass));
    if (window < 1 || window > VC_TEMPORAL_MAX_WINDOW)
        return fail(ctx, VC_ERR_ARG, "vc_hull_temporal: window %u not in [1, %u]", window, VC_TEMPORAL_MAX_WINDOW);
    if (keep_on < 1 || keep_on > window) return fail(ctx, VC_ERR_ARG, "vc_hull_temporal: keep_on %u not in [1, window = %u]", keep_on, window);
    if (keep_off < 1 || keep_off > keep_on)
        return fail(ctx, VC_ERR_ARG, "vc_hull_temporal: keep_off %u not in [1, keep_on = %u]", keep_off, keep_on);
    StepBuf &cur = *pass.cur;
    const uint64_t n = pass.n, nwords = pass.nwords, npad = (nwords + 1) & ~1ull;
    VC_TRY(merge_refuse_index(ctx, "vc_hull_temporal", n));
    VC_TRY(merge_refuse_slot(ctx, "vc_hull_temporal", cur));
    vc_ctx::Temporal &T = ctx->temporal;
    if (ctx->current(T.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_hull_temporal: the current result is already the last call's output (one push per result): carve again first");
    if (!n || cur.words.cap < npad) return fail(ctx, VC_ERR_INTERNAL, "vc_hull_temporal: the result's %llu occupancy words are not padded to %llu",
                                                (unsigned long long)cur.words.cap, (unsigned long long)npad);
    VC_TRY(pass_begin(ctx));
    // a ring of another window or another grid starts over; its buffers are made beside the old ones, which stay until the call commits
    const bool restart = T.pushes == 0 || T.window != window || T.nwords != nwords || T.aligned;
    const bool alloc = T.ring.cap < (size_t)window * npad || T.prev.cap < npad || T.stage.cap < npad || !T.ring.ptr;
    DevBuf<uint64_t> ring2, prev2, stage2;
    if (alloc) {
        if (!restart) return fail(ctx, VC_ERR_INTERNAL, "vc_hull_temporal: the ring holds %zu words, %u x %llu are in use", T.ring.cap, window,
                                  (unsigned long long)npad);
        VC_TRY(ensure(ctx, ring2, (size_t)window * npad));
        VC_TRY(ensure(ctx, prev2, (size_t)npad));
        VC_TRY(ensure(ctx, stage2, (size_t)npad));
    }
    VC_TRY(ensure(ctx, T.ctr, 8));
    VC_HIP(ctx, ensure_pinned(T.h, 8));
    const uint64_t have = restart ? 0 : std::min<uint64_t>(T.pushes, window);     // snapshots in the ring
    const uint32_t m = (uint32_t)std::min<uint64_t>(have + 1, window);
    const uint32_t on = (keep_on * m + window - 1) / window, off = (keep_off * m + window - 1) / window;
    const uint64_t S0 = pass.S;
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    TemporalParams tp;
    memset(&tp, 0, sizeof tp);
    tp.ring = alloc ? ring2.ptr : T.ring.ptr;
    tp.cur = cur.words.ptr;
    tp.prev = restart ? nullptr : T.prev.ptr;
    tp.stage = alloc ? stage2.ptr : T.stage.ptr;
    tp.ctr = T.ctr.ptr;
    tp.nwords = nwords; tp.npad = npad; tp.n = n;
    tp.window = window; tp.head = restart ? 0 : T.head;
    tp.count = m - 1;                            // (the ring's oldest slot is read only when the ring is not yet full)
    tp.on = on; tp.off = off;
    const dim3 vblock(kTemporalBlock), vgrid((uint32_t)((npad / 2 + kTemporalBlock - 1) / kTemporalBlock));
    VC_HIP(ctx, hipMemsetAsync(T.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    VC_DLAUNCH(VC_K_TEMPORAL_VOTE, k_temporal_vote, vgrid, vblock, tp);
    VC_HIP(ctx, hipGetLastError());
    // the read-back in the middle: |O_t| sizes the records
    VC_HIP(ctx, hipMemcpyAsync(T.h.ptr, T.ctr.ptr, kTemporalCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t S1 = T.h[0], added = T.h[1], removed = T.h[2], raw_changed = T.h[3], out_changed = T.h[4];
    if (S1 > n || removed > S0 || S0 + added - removed != S1)
        return fail(ctx, VC_ERR_HIP, "vc_hull_temporal: %llu voted in, %llu added to and %llu removed from %llu survivors, in a grid of %llu voxels",
                    (unsigned long long)S1, (unsigned long long)added, (unsigned long long)removed, (unsigned long long)S0, (unsigned long long)n);
    const bool changed = added || removed;
    // every buffer of the hand-over before anything is committed: a failure leaves result, ring and P
    VC_TRY(ensure(ctx, T.votes, (size_t)S1));
    VC_TRY(ensure(ctx, T.added, (size_t)S1));
    MergeParams g;
    VC_TRY(merge_sized(ctx, cur, nwords, S1, changed, T.added.ptr, g));
    // committed from here on: the ring takes H_t, the result O_t, P the staging buffer
    T.stamp = kNever;
    if (alloc) { T.ring = std::move(ring2); T.prev = std::move(prev2); T.stage = std::move(stage2); }
    if (restart) {
        VC_HIP(ctx, hipMemsetAsync(T.ring.ptr, 0, (size_t)window * npad * sizeof(uint64_t), ctx->stream));   // (the slots' pads stay zero)
        T.window = window; T.nwords = nwords; T.npad = npad;
        T.head = window - 1;
        T.pushes = 0;
        T.aligned = false;
        T.ring2.reset();                         // (the second ring of vc_hull_temporal_motion: this ring has no use for it)
    }
    T.has_field = false;
    T.head = (T.head + 1) % window;
    T.pushes += 1;
    VC_HIP(ctx, hipMemcpyAsync(T.ring.ptr + (size_t)T.head * npad, cur.words.ptr, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(T.added.ptr, 0, std::max<size_t>((size_t)S1, 1), ctx->stream));
    tp.ring = T.ring.ptr; tp.head = T.head; tp.count = m; tp.cur = nullptr; tp.prev = nullptr;
    const dim3 gblock(kMergeBlock), wgrid((uint32_t)((nwords + kMergeBlock - 1) / kMergeBlock));
    if (changed) {
        result_changed(ctx);
        VC_HIP(ctx, hipMemcpyAsync(cur.words.ptr, tp.stage, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (changed || S1) VC_TRY(merge_ranked(ctx, cur, g, nwords, S0, changed, VC_K_TEMPORAL_RANK, VC_K_TEMPORAL_MERGE));
    // the vote byte of every record of O_t and a fresh record for every restored voxel; or O_t = H_t: records, occupancy and every
    // product of a pass stay, only the vote bytes are made
    if (changed && S1) VC_DLAUNCH(VC_K_TEMPORAL_MERGE, k_temporal_new<true>, wgrid, gblock, g, tp, T.votes.ptr);
    else if (S1) VC_DLAUNCH(VC_K_TEMPORAL_RANK, k_temporal_new<false>, wgrid, gblock, g, tp, T.votes.ptr);
    VC_HIP(ctx, hipGetLastError());
    if (changed) VC_TRY(records_handed_over(ctx, cur, word_groups(nwords)));
    std::swap(T.prev, T.stage);                  // (the launches above hold the pointers they were given)
    VC_TRY(pass_end(ctx, pass, &stats->temporal_ms));
    if (changed) ctx->survivors = cur.survivors = S1;
    if (changed || S1) VC_TRY(merge_counted(ctx, "vc_hull_temporal", S1, "were voted in"));
    stats->window = window; stats->frames = m; stats->on = on; stats->off = off;
    stats->survivors_before = S0; stats->survivors_after = S1;
    stats->added = added; stats->removed = removed;
    stats->raw_changed = raw_changed; stats->out_changed = out_changed;
    T.stamp = ctx->result_gen;
    T.n = S1;
    return VC_OK;
}

int vc_fetch_temporal(vc_ctx *ctx, uint8_t *votes, uint8_t *added)
{
    if (!ctx) return VC_ERR_ARG;
    const vc_ctx::Temporal &T = ctx->temporal;
    if (!ctx->carved || !ctx->current(T.stamp)) return fail(ctx, VC_ERR_ARG, "no votes: call vc_hull_temporal on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (votes && T.n) VC_HIP(ctx, hipMemcpy(votes, T.votes.ptr, (size_t)T.n, hipMemcpyDeviceToHost));
    if (added && T.n) VC_HIP(ctx, hipMemcpy(added, T.added.ptr, (size_t)T.n, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_temporal_history(vc_ctx *ctx, uint32_t age, uint8_t *bits)
{
    if (!ctx || !bits) return VC_ERR_ARG;
    const vc_ctx::Temporal &T = ctx->temporal;
    const uint64_t m = std::min<uint64_t>(T.pushes, T.window);
    if (age >= m) return fail(ctx, VC_ERR_ARG, "vc_fetch_temporal_history: age %u, the ring holds %llu hulls", age, (unsigned long long)m);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t slot = (T.head + T.window - age) % T.window;
    VC_HIP(ctx, hipMemcpy(bits, T.ring.ptr + (size_t)slot * T.npad, (size_t)T.nwords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_temporal_reset(vc_ctx *ctx)
{
    if (!ctx) return VC_ERR_ARG;
    ctx->temporal.pushes = 0;
    ctx->temporal.stamp = kNever;
    return VC_OK;
}

// ---- set algebra on hulls: kept hulls, combine, compare (vc_setops.h; contract in include/voxcarve.h) ----
// Register `reg` holds another hull (or none) from here on: a motion field made against it is stale.
static void motion_reg_written(vc_ctx *ctx, uint32_t reg)
{
    if (ctx->motion.reg == reg) ctx->motion.stamp = kNever;
}

// The refusals of the calls that name a register; `filled`: the register must hold a hull.
static int kept_refusals(vc_ctx *ctx, const char *what, uint32_t reg, bool filled)
{
    if (reg >= VC_HULL_REGISTERS) return fail(ctx, VC_ERR_ARG, "%s: register %u, there are %u", what, reg, (unsigned)VC_HULL_REGISTERS);
    if (filled && !ctx->setops.reg[reg].used) return fail(ctx, VC_ERR_ARG, "%s: register %u is empty", what, reg);
    return VC_OK;
}

static dim3 setop_pairs(uint64_t npad) { return dim3((uint32_t)((npad / 2 + kSetopBlock - 1) / kSetopBlock)); }

// Queues count and check of staged occupancy words: ctr[0] = their voxels, ctr[1] += 1 per word with a bit at or beyond n.
static int kept_count(vc_ctx *ctx, const uint64_t *words, uint64_t nwords, uint64_t n)
{
    hipLaunchKernelGGL(k_kept_bits, dim3((uint32_t)((nwords + kSetopBlock - 1) / kSetopBlock)), dim3(kSetopBlock), 0, ctx->stream, words, nwords, n,
                       ctx->setops.ctr.ptr);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

int vc_hull_keep(vc_ctx *ctx, uint32_t reg)
{
    if (!ctx) return VC_ERR_ARG;
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_keep", "keep", "hull registers", pass));
    VC_TRY(kept_refusals(ctx, "vc_hull_keep", reg, false));
    VC_TRY(merge_refuse_index(ctx, "vc_hull_keep", pass.n));
    StepBuf &cur = *pass.cur;
    const uint64_t n = pass.n, nwords = pass.nwords, npad = (nwords + 1) & ~1ull, S = pass.S;
    if (!n || cur.words.cap < npad) return fail(ctx, VC_ERR_INTERNAL, "vc_hull_keep: the result's %llu occupancy words are not padded to %llu",
                                                (unsigned long long)cur.words.cap, (unsigned long long)npad);
    vc_ctx::Setops &X = ctx->setops;
    VC_TRY(pass_begin(ctx));
    vc_ctx::Kept k;                              // built beside the register, which stays as it is until the copy is whole
    VC_TRY(ensure(ctx, k.words, (size_t)npad));
    VC_TRY(ensure(ctx, k.rec, (size_t)S));
    VC_TRY(ensure(ctx, X.ctr, 8));
    VC_HIP(ctx, ensure_pinned(X.h, 16));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    // R = the result's valid bits, pad included, by the combine's own kernel (a = b = the result's words, COPY)
    SetopParams sp;
    memset(&sp, 0, sizeof sp);
    sp.a = sp.b = cur.words.ptr; sp.stage = k.words.ptr; sp.ctr = X.ctr.ptr;
    sp.nwords = nwords; sp.n = n; sp.op = kSetopCopy;
    VC_HIP(ctx, hipMemsetAsync(X.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_setop_words, setop_pairs(npad), dim3(kSetopBlock), 0, ctx->stream, sp);
    VC_HIP(ctx, hipGetLastError());
    if (S) VC_HIP(ctx, hipMemcpyAsync(k.rec.ptr, cur.records.ptr, (size_t)S * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    VC_HIP(ctx, hipMemcpyAsync(X.h.ptr, X.ctr.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, nullptr));
    if (X.h[0] != S) return fail(ctx, VC_ERR_HIP, "vc_hull_keep: the occupancy holds %llu voxels, the result %llu records", (unsigned long long)X.h[0],
                                 (unsigned long long)S);
    k.count = S; k.used = true; k.has_rec = true;
    X.reg[reg] = std::move(k);
    motion_reg_written(ctx, reg);
    return VC_OK;
}

int vc_hull_upload(vc_ctx *ctx, uint32_t reg, const uint8_t *bits, const uint64_t *records, uint64_t n_records)
{
    if (!ctx) return VC_ERR_ARG;
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->have_grid) return fail(ctx, VC_ERR_ARG, "vc_hull_upload: no grid");
    if (ctx->z0 != 0 || ctx->z1 != ctx->nz)
        return fail(ctx, VC_ERR_ARG, "vc_hull_upload: the slab [%u,%u) is narrower than the grid's %u layers", ctx->z0, ctx->z1, ctx->nz);
    VC_TRY(kept_refusals(ctx, "vc_hull_upload", reg, false));
    if ((bits != nullptr) == (records != nullptr)) return fail(ctx, VC_ERR_ARG, "vc_hull_upload: exactly one of bits and records must be given");
    if (bits && n_records) return fail(ctx, VC_ERR_ARG, "vc_hull_upload: n_records = %llu with bits", (unsigned long long)n_records);
    const uint64_t n = ctx->n_voxels(), nwords = (n + 63) / 64, npad = (nwords + 1) & ~1ull;
    if (!n) return fail(ctx, VC_ERR_ARG, "vc_hull_upload: the grid has no voxels");
    VC_TRY(merge_refuse_index(ctx, "vc_hull_upload", n));
    if (n_records > n) return fail(ctx, VC_ERR_ARG, "vc_hull_upload: %llu records in a grid of %llu voxels", (unsigned long long)n_records, (unsigned long long)n);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    vc_ctx::Setops &X = ctx->setops;
    vc_ctx::Kept k;                              // the hull is built here and swapped in only when it is valid
    VC_TRY(ensure(ctx, k.words, (size_t)npad));
    if (records) VC_TRY(ensure(ctx, k.rec, (size_t)n_records));
    VC_TRY(ensure(ctx, X.ctr, 8));
    VC_HIP(ctx, ensure_pinned(X.h, 16));
    VC_HIP(ctx, hipMemsetAsync(X.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(k.words.ptr, 0, (size_t)npad * sizeof(uint64_t), ctx->stream));
    if (bits) {
        VC_HIP(ctx, hipMemcpyAsync(k.words.ptr, bits, (size_t)nwords * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    } else if (n_records) {
        VC_HIP(ctx, hipMemcpyAsync(k.rec.ptr, records, (size_t)n_records * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_kept_records, dim3((uint32_t)((n_records + kSetopBlock - 1) / kSetopBlock)), dim3(kSetopBlock), 0, ctx->stream,
                           (const uint64_t *)k.rec.ptr, n_records, nwords, n, reinterpret_cast<unsigned long long *>(k.words.ptr), X.ctr.ptr);
        VC_HIP(ctx, hipGetLastError());
    }
    VC_TRY(kept_count(ctx, k.words.ptr, nwords, n));
    VC_HIP(ctx, hipMemcpyAsync(X.h.ptr, X.ctr.ptr, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (X.h[1] && bits)
        return fail(ctx, VC_ERR_ARG, "vc_hull_upload: %llu words hold a bit at or beyond the grid's %llu voxels", (unsigned long long)X.h[1],
                    (unsigned long long)n);
    if (X.h[1])
        return fail(ctx, VC_ERR_ARG, "vc_hull_upload: %llu records are out of order, duplicates or at or beyond the grid's %llu voxels",
                    (unsigned long long)X.h[1], (unsigned long long)n);
    if (records && X.h[0] != n_records)
        return fail(ctx, VC_ERR_HIP, "vc_hull_upload: %llu bits from %llu records", (unsigned long long)X.h[0], (unsigned long long)n_records);
    k.count = X.h[0]; k.used = true; k.has_rec = records != nullptr;
    X.reg[reg] = std::move(k);
    motion_reg_written(ctx, reg);
    return VC_OK;
}

int vc_hull_release(vc_ctx *ctx, uint32_t reg)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(kept_refusals(ctx, "vc_hull_release", reg, false));
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->setops.reg[reg] = vc_ctx::Kept{};
    motion_reg_written(ctx, reg);
    return VC_OK;
}

int vc_fetch_kept(vc_ctx *ctx, uint32_t reg, uint8_t *bits, uint64_t *records, uint64_t *count, uint32_t *has_records)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(kept_refusals(ctx, "vc_fetch_kept", reg, true));
    const vc_ctx::Kept &k = ctx->setops.reg[reg];
    if (records && !k.has_rec) return fail(ctx, VC_ERR_ARG, "vc_fetch_kept: register %u holds no records", reg);
    if (count) *count = k.count;
    if (has_records) *has_records = k.has_rec ? 1u : 0u;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t nwords = (ctx->n_voxels() + 63) / 64;
    if (bits && nwords) VC_HIP(ctx, hipMemcpy(bits, k.words.ptr, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (records && k.count) VC_HIP(ctx, hipMemcpy(records, k.rec.ptr, (size_t)k.count * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_hull_combine(vc_ctx *ctx, uint32_t op, uint32_t reg, uint32_t flags, vc_setop_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_combine: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_combine", "combine", "set operations", pass));
    if (op > VC_SETOP_XOR) return fail(ctx, VC_ERR_ARG, "vc_hull_combine: unknown op %u (VC_SETOP_COPY .. VC_SETOP_XOR)", op);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_combine: flags must be 0 (got %u)", flags);
    VC_TRY(kept_refusals(ctx, "vc_hull_combine", reg, true));
    StepBuf &cur = *pass.cur;
    const uint64_t n = pass.n, nwords = pass.nwords, npad = (nwords + 1) & ~1ull;
    VC_TRY(merge_refuse_index(ctx, "vc_hull_combine", n));
    vc_ctx::Setops &X = ctx->setops;
    const vc_ctx::Kept &B = X.reg[reg];
    const bool colours = !B.has_rec && (op == VC_SETOP_COPY || op == VC_SETOP_OR || op == VC_SETOP_XOR);   // fresh records may be made
    if (colours) VC_TRY(merge_refuse_slot(ctx, "vc_hull_combine", cur));
    if (!n || cur.words.cap < npad || B.words.cap < npad)
        return fail(ctx, VC_ERR_INTERNAL, "vc_hull_combine: %llu and %llu occupancy words are not padded to %llu", (unsigned long long)cur.words.cap,
                    (unsigned long long)B.words.cap, (unsigned long long)npad);
    VC_TRY(pass_begin(ctx));
    VC_TRY(ensure(ctx, X.stage, (size_t)npad));
    VC_TRY(ensure(ctx, X.ctr, 8));
    VC_HIP(ctx, ensure_pinned(X.h, 16));
    const uint64_t S0 = pass.S;
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    SetopParams sp;
    memset(&sp, 0, sizeof sp);
    sp.a = cur.words.ptr; sp.b = B.words.ptr; sp.stage = X.stage.ptr; sp.ctr = X.ctr.ptr;
    sp.nwords = nwords; sp.n = n; sp.op = op;
    VC_HIP(ctx, hipMemsetAsync(X.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_setop_words, setop_pairs(npad), dim3(kSetopBlock), 0, ctx->stream, sp);
    VC_HIP(ctx, hipGetLastError());
    // the read-back in the middle: |R| sizes the records
    VC_HIP(ctx, hipMemcpyAsync(X.h.ptr, X.ctr.ptr, kSetopCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t S1 = X.h[0], common = X.h[1], added = X.h[2], removed = X.h[3];
    if (S1 > n || removed > S0 || S0 + added - removed != S1 || common > S0 || common > B.count)
        return fail(ctx, VC_ERR_HIP, "vc_hull_combine: %llu in the result, %llu common, %llu added to and %llu removed from %llu survivors, in a grid of %llu voxels",
                    (unsigned long long)S1, (unsigned long long)common, (unsigned long long)added, (unsigned long long)removed, (unsigned long long)S0,
                    (unsigned long long)n);
    const bool restore = op == VC_SETOP_COPY && B.has_rec;      // every record becomes B's: their bytes may differ where the sets do not
    const bool changed = added || removed || restore;
    // every buffer of the hand-over before anything is committed: a failure leaves result and registers
    VC_TRY(ensure(ctx, X.added, (size_t)S1));
    MergeParams g;
    VC_TRY(merge_sized(ctx, cur, nwords, S1, changed, X.added.ptr, g));
    // committed from here on
    X.stamp = kNever;
    VC_HIP(ctx, hipMemsetAsync(X.added.ptr, 0, std::max<size_t>((size_t)S1, 1), ctx->stream));
    if (changed) {
        result_changed(ctx);
        // R into the result's words; where voxels were added the staging buffer takes A's words for the kernels that ask which are new
        if (added) hipLaunchKernelGGL(k_setop_commit, setop_pairs(npad), dim3(kSetopBlock), 0, ctx->stream, cur.words.ptr, X.stage.ptr, nwords, n);
        else VC_HIP(ctx, hipMemcpyAsync(cur.words.ptr, X.stage.ptr, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        VC_HIP(ctx, hipGetLastError());
        VC_TRY(merge_ranked(ctx, cur, g, nwords, restore ? 0 : S0, true, -1, -1));   // (a restore moves no record of A)
        const uint64_t *olda = added ? X.stage.ptr : nullptr;
        if (B.has_rec && B.count && (added || restore))
            hipLaunchKernelGGL(k_merge_from, dim3((uint32_t)((B.count + kMergeBlock - 1) / kMergeBlock)), dim3(kMergeBlock), 0, ctx->stream, g,
                               (const uint64_t *)B.rec.ptr, B.count, nwords, olda, restore ? 1 : 0);
        else if (!B.has_rec && added)
            hipLaunchKernelGGL(k_setop_fresh, dim3((uint32_t)((nwords + kMergeBlock - 1) / kMergeBlock)), dim3(kMergeBlock), 0, ctx->stream, g, olda,
                               nwords, n);
        VC_HIP(ctx, hipGetLastError());
        VC_TRY(records_handed_over(ctx, cur, word_groups(nwords)));
    }
    VC_TRY(pass_end(ctx, pass, &stats->setop_ms));
    if (changed) {
        ctx->survivors = cur.survivors = S1;
        VC_TRY(merge_counted(ctx, "vc_hull_combine", S1, "were combined"));
    }
    stats->survivors_before = S0; stats->other = B.count; stats->common = common;
    stats->survivors_after = S1; stats->added = added; stats->removed = removed;
    X.stamp = ctx->result_gen;
    X.n = S1;
    return VC_OK;
}

int vc_fetch_combined(vc_ctx *ctx, uint8_t *added)
{
    if (!ctx || !added) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->setops.stamp)) return fail(ctx, VC_ERR_ARG, "no added flags: call vc_hull_combine on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->setops.n) VC_HIP(ctx, hipMemcpy(added, ctx->setops.added.ptr, (size_t)ctx->setops.n, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_hull_compare(vc_ctx *ctx, uint32_t reg, uint32_t flags, vc_compare_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_compare: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_compare", "compare", "comparison", pass));
    if (flags & ~VC_COMPARE_DISTANCE) return fail(ctx, VC_ERR_ARG, "vc_hull_compare: unknown flags %u (VC_COMPARE_DISTANCE)", flags);
    VC_TRY(kept_refusals(ctx, "vc_hull_compare", reg, true));
    const bool distance = (flags & VC_COMPARE_DISTANCE) != 0;
    uint64_t q[3] = {0, 0, 0};
    if (distance) VC_TRY(dist_metric(ctx, "vc_hull_compare", q));
    StepBuf &cur = *pass.cur;
    const uint64_t n = pass.n, nwords = pass.nwords, npad = (nwords + 1) & ~1ull;
    VC_TRY(merge_refuse_index(ctx, "vc_hull_compare", n));
    vc_ctx::Setops &X = ctx->setops;
    const vc_ctx::Kept &B = X.reg[reg];
    if (!n || cur.words.cap < npad || B.words.cap < npad)
        return fail(ctx, VC_ERR_INTERNAL, "vc_hull_compare: %llu and %llu occupancy words are not padded to %llu", (unsigned long long)cur.words.cap,
                    (unsigned long long)B.words.cap, (unsigned long long)npad);
    VC_TRY(pass_begin(ctx));
    VC_TRY(ensure(ctx, X.ctr, 8));
    VC_TRY(ensure(ctx, X.box, 12));
    VC_TRY(ensure(ctx, X.acc, 4));
    VC_HIP(ctx, ensure_pinned(X.h, 16));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    uint32_t *hb = reinterpret_cast<uint32_t *>(X.h.ptr + 4);    // h[0..2]: the counts; h[4..9]: the boxes; h[10..13]: the maxima
    for (int k = 0; k < 12; ++k) hb[k] = (k % 6) < 3 ? 0xffffffffu : 0u;
    VC_HIP(ctx, hipMemcpyAsync(X.box.ptr, hb, 12 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(X.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    CompareParams cp;
    memset(&cp, 0, sizeof cp);
    cp.a = cur.words.ptr; cp.b = B.words.ptr; cp.ctr = X.ctr.ptr; cp.box = X.box.ptr;
    cp.nwords = nwords; cp.n = n; cp.nx = ctx->nx; cp.ny = ctx->ny; cp.nz = ctx->nz;
    hipLaunchKernelGGL(k_compare_words, setop_pairs(npad), dim3(kSetopBlock), 0, ctx->stream, cp);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(X.h.ptr, X.ctr.ptr, kCompareCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipMemcpyAsync(hb, X.box.ptr, 12 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t common = X.h[0], only_a = X.h[1], only_b = X.h[2];
    if (common + only_a != pass.S || common + only_b != B.count)
        return fail(ctx, VC_ERR_HIP, "vc_hull_compare: %llu common, %llu and %llu one-sided voxels of hulls of %llu and %llu", (unsigned long long)common,
                    (unsigned long long)only_a, (unsigned long long)only_b, (unsigned long long)pass.S, (unsigned long long)B.count);
    const uint32_t dims[3] = {ctx->nx, ctx->ny, ctx->nz};
    uint32_t diff[6], uni[6];
    memcpy(diff, hb, sizeof diff);
    memcpy(uni, hb + 6, sizeof uni);
    if (only_a + only_b)
        for (int a = 0; a < 3; ++a)
            if (diff[a] > diff[3 + a] || diff[3 + a] >= dims[a] || uni[a] > diff[a] || uni[3 + a] < diff[3 + a] || uni[3 + a] >= dims[a])
                return fail(ctx, VC_ERR_HIP, "vc_hull_compare: the difference's box [%u, %u] in the union's [%u, %u] on axis %c of %u cells", diff[a],
                            diff[3 + a], uni[a], uni[3 + a], "xyz"[a], dims[a]);
    uint64_t *hm = X.h.ptr + 10;
    hm[0] = hm[2] = 0; hm[1] = hm[3] = 0xffffffffull;
    if (distance && (only_a || only_b)) {
        // two transforms over the union's index box, grown by a cell per side and clipped to the grid: every site of either hull lies
        // inside it, so the minima are exact; sites = B for the voxels of A \ B, then sites = A for those of B \ A
        DistBox bx;
        memset(&bx, 0, sizeof bx);
        bx.nx = ctx->nx; bx.ny = ctx->ny; bx.nz = ctx->nz;
        for (int a = 0; a < 3; ++a) {
            const int32_t lo = uni[a] ? (int32_t)uni[a] - 1 : 0, hi = std::min<int32_t>((int32_t)uni[3 + a] + 1, (int32_t)dims[a] - 1);
            bx.o[a] = lo;
            bx.b[a] = (uint32_t)(hi - lo + 1);
        }
        VC_TRY(dist_ensure(ctx, X.field, bx));
        VC_HIP(ctx, hipMemcpyAsync(X.acc.ptr, hm, 4 * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        const dim3 wgrid((uint32_t)((nwords + kSetopBlock - 1) / kSetopBlock)), block(kSetopBlock);
        for (int dir = 0; dir < 2; ++dir) {
            if (!(dir ? only_b : only_a)) continue;
            const uint64_t *x = dir ? B.words.ptr : cur.words.ptr, *y = dir ? cur.words.ptr : B.words.ptr;
            VC_TRY(dist_transform(ctx, bx, kDistSiteOn, y, X.field.ptr, 0, q));
            hipLaunchKernelGGL(k_compare_far<false>, wgrid, block, 0, ctx->stream, bx, (const uint64_t *)X.field.ptr, x, y, nwords, n, X.acc.ptr + 2 * dir);
            hipLaunchKernelGGL(k_compare_far<true>, wgrid, block, 0, ctx->stream, bx, (const uint64_t *)X.field.ptr, x, y, nwords, n, X.acc.ptr + 2 * dir);
            VC_HIP(ctx, hipGetLastError());
        }
        VC_TRY(pass_stop(ctx, pass));
        VC_HIP(ctx, hipMemcpyAsync(hm, X.acc.ptr, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    VC_TRY(pass_end(ctx, pass, &stats->compare_ms));
    stats->a = pass.S; stats->b = B.count; stats->common = common; stats->only_a = only_a; stats->only_b = only_b;
    for (int a = 0; a < 3; ++a) { stats->diff_lo[a] = diff[a]; stats->diff_hi[a] = diff[3 + a]; stats->q[a] = q[a]; }
    stats->h2_ab = hm[0]; stats->arg_ab = (uint32_t)hm[1];
    stats->h2_ba = hm[2]; stats->arg_ba = (uint32_t)hm[3];
    return VC_OK;
}

// From here on the host side of a family lives beside its kernels in a file of its own under host/, included once, in dependency
// order (still this one translation unit: a file may use what stands above it).
#include "host/motion.h"     // vc_hull_motion, vc_hull_warp, vc_paint_motion (the kept hulls of the set algebra above)
#include "host/motion_pyramid.h"    // vc_hull_motion_pyramid and its per-level fetches (motion_grid, motion_listed and motion_field of motion.h)
#include "host/temporal_motion.h"   // vc_hull_temporal_motion (the vote's ring and hand-over above, motion_field of motion.h)
#include "host/render.h"     // vc_render, vc_fetch_render (the pass frame above); the colouring pass's vc_fetch_visibility, vc_fetch_depth
#include "host/mc.h"         // vc_marching_cubes over the dense volume (densify_words and scan_counts above)
#include "host/surface.h"    // vc_surface_mesh: the silhouette-refined mesh (scan_counts above)
#include "host/normals.h"    // vc_hull_normals, vc_shade_render, vc_surface_normals (dist_metric and isqrt_u64 of the distance and grow passes above)
#include "host/texture.h"    // vc_texture_render (the last render of render.h; visible_start of the colouring pass above)
#include "host/light.h"      // vc_light_render: shadows, ambient occlusion, floor (the last render of render.h)
#include "host/clusters.h"   // vc_hull_clusters (dist_metric of the distance passes above)
#include "host/geodesic.h"   // vc_hull_geodesic, extremities, paths (dist_metric and the survivors' box of the distance passes above)
#include "host/measure.h"    // vc_hull_measure (the labels of clusters.h and geodesic.h); ms_divisor
#include "host/shell.h"      // vc_hull_shell (ms_divisor of measure.h, as vc_shell.h takes ms_div from vc_measure.h)
#include "host/thin.h"       // vc_hull_thin (ms_divisor of measure.h, as vc_thin.h takes ms_div from vc_measure.h)

// ---- the step before the path, its data-parallel part (reference background_subtraction.py:153-168) ----
static int hsv_tables(vc_ctx *ctx);

int vc_bgr_to_hsv(vc_ctx *ctx, const uint8_t *bgr, uint32_t H, uint32_t W, uint8_t *hsv)
{
    if (!ctx || !bgr || !hsv) return VC_ERR_ARG;
    if (H == 0 || W == 0 || (uint64_t)H * W > 0x3fffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u", H, W);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(hsv_tables(ctx));
    VC_TRY(ensure(ctx, ctx->d_fg, npix * 6 + 64));
    uint8_t *d_in = ctx->d_fg.ptr, *d_out = d_in + npix * 3;
    VC_HIP(ctx, hipMemcpyAsync(d_in, bgr, npix * 3, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bgr2hsv, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_in, d_out, (uint32_t)npix,
                       (const int32_t *)ctx->d_hsvdiv.ptr, (const int32_t *)(ctx->d_hsvdiv.ptr + 256));
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(hsv, d_out, npix * 3, hipMemcpyDeviceToHost, st));
    VC_HIP(ctx, hipStreamSynchronize(st));
    return VC_OK;
}

int vc_mask_morphology(vc_ctx *ctx, const uint8_t *mask, uint32_t H, uint32_t W, uint32_t ksize, int open, int close, uint8_t *out)
{
    if (!ctx || !mask || !out) return VC_ERR_ARG;
    if (ksize != 2 && ksize != 3) return fail(ctx, VC_ERR_ARG, "structuring element %u x %u: the reference uses 3 x 3 (pre) and 2 x 2 (post)", ksize, ksize);
    if (H == 0 || W == 0 || (uint64_t)H * W > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u", H, W);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(ensure(ctx, ctx->d_fg, npix * 6 + 64));
    uint8_t *a = ctx->d_fg.ptr, *b = a + npix;
    VC_HIP(ctx, hipMemcpyAsync(a, mask, npix, hipMemcpyHostToDevice, st));
    const dim3 g((uint32_t)((npix + 255) / 256)), blk(256);
    auto pass = [&](bool dilate) {                               // a -> b, then the two swap
        if (ksize == 3) {
            if (dilate) hipLaunchKernelGGL(k_morph3x3<true>, g, blk, 0, st, (const uint8_t *)a, b, H, W);
            else hipLaunchKernelGGL(k_morph3x3<false>, g, blk, 0, st, (const uint8_t *)a, b, H, W);
        } else {
            if (dilate) hipLaunchKernelGGL(k_morph2x2<true>, g, blk, 0, st, (const uint8_t *)a, b, H, W);
            else hipLaunchKernelGGL(k_morph2x2<false>, g, blk, 0, st, (const uint8_t *)a, b, H, W);
        }
        uint8_t *t = a; a = b; b = t;
    };
    if (open) { pass(false); pass(true); }                       // MORPH_OPEN = erode, dilate
    if (close) { pass(true); pass(false); }                      // MORPH_CLOSE = dilate, erode (opening first when both are asked)
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(out, a, npix, hipMemcpyDeviceToHost, st));
    VC_HIP(ctx, hipStreamSynchronize(st));
    return VC_OK;
}

int vc_mog_create(vc_ctx *ctx, int history, int nmixtures, double background_ratio, double noise_sigma, uint32_t *model)
{
    if (!ctx || !model) return VC_ERR_ARG;
    for (uint32_t i = 0; i < VC_MAX_MOG_MODELS; ++i) {
        vc_ctx::MogModel &m = ctx->mog[i];
        if (m.used) continue;
        // the constructor's clamps (bgfg_gaussmix.cpp, BackgroundSubtractorMOGImpl): non-positive arguments select the defaults
        m.nmixtures = nmixtures > 0 ? nmixtures : 5;
        if (m.nmixtures > kMogMaxMixtures) m.nmixtures = kMogMaxMixtures;
        m.history = history > 0 ? history : 200;
        m.background_ratio = background_ratio > 0 ? background_ratio : 0.95;
        if (m.background_ratio > 1.0) m.background_ratio = 1.0;
        m.noise_sigma = noise_sigma <= 0 ? 15.0 : noise_sigma;
        m.H = m.W = m.nframes = 0;
        m.used = true;
        *model = i;
        return VC_OK;
    }
    return fail(ctx, VC_ERR_ARG, "all %d background models of this context are in use", VC_MAX_MOG_MODELS);
}

int vc_mog_destroy(vc_ctx *ctx, uint32_t model)
{
    if (!ctx) return VC_ERR_ARG;
    if (model >= VC_MAX_MOG_MODELS || !ctx->mog[model].used) return fail(ctx, VC_ERR_ARG, "no background model %u", model);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
    ctx->mog[model].state.reset();
    ctx->mog[model].used = false;
    return VC_OK;
}

// One frame through a background model: d_img (device, [H W 3]) -> d_mask (device, [H W]) on the upload stream.
static int mog_enqueue(vc_ctx *ctx, uint32_t model, const uint8_t *d_img, uint32_t H, uint32_t W, double learning_rate, uint8_t *d_mask)
{
    vc_ctx::MogModel &m = ctx->mog[model];
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    // apply(): the model starts over on its first frame, on a learning rate >= 1 and when the image size changes
    if (m.nframes == 0 || learning_rate >= 1 || m.H != H || m.W != W) {
        VC_TRY(ensure(ctx, m.state, npix * 8 * (size_t)m.nmixtures));
        VC_HIP(ctx, hipMemsetAsync(m.state.ptr, 0, npix * 8 * (size_t)m.nmixtures * sizeof(float), st));
        m.H = H; m.W = W; m.nframes = 0;
    }
    ++m.nframes;
    const double lr = learning_rate >= 0 && m.nframes > 1 ? learning_rate : 1.0 / (double)(m.nframes < (uint32_t)m.history ? m.nframes : (uint32_t)m.history);
    const double default_noise_sigma = 30 * 0.5, w0 = 0.05;
    MogParams p;
    p.alpha = (float)lr; p.T = (float)m.background_ratio; p.vT = (float)(2.5 * 2.5);
    p.w0 = (float)w0;
    p.sk0 = (float)(w0 / (default_noise_sigma * 2 * std::sqrt(3.)));
    p.var0 = (float)(default_noise_sigma * default_noise_sigma * 4);
    p.minVar = (float)(m.noise_sigma * m.noise_sigma);
    p.K = (uint32_t)m.nmixtures; p.npix = (uint32_t)npix;
    hipLaunchKernelGGL(k_mog_apply, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, d_img, d_mask, m.state.ptr, p);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// MOG2 handles carry VC_MOG2_MODEL_TAG over their own table; a MOG handle is the bare index.
static vc_ctx::Mog2Model *mog2_model(vc_ctx *ctx, uint32_t model)
{
    if ((model & ~(uint32_t)(VC_MOG2_MODEL_TAG - 1)) != VC_MOG2_MODEL_TAG) return nullptr;
    const uint32_t i = model & (VC_MOG2_MODEL_TAG - 1);
    return i < VC_MAX_MOG_MODELS && ctx->mog2[i].used ? &ctx->mog2[i] : nullptr;
}

static bool any_model(vc_ctx *ctx, uint32_t model)
{
    return (model < VC_MAX_MOG_MODELS && ctx->mog[model].used) || mog2_model(ctx, model) != nullptr;
}

int vc_mog2_create(vc_ctx *ctx, int history, double var_threshold, int detect_shadows, int nmixtures, double background_ratio,
                   double var_threshold_gen, double var_init, double var_min, double var_max, double complexity_reduction_threshold,
                   int shadow_value, double shadow_threshold, uint32_t *model)
{
    if (!ctx || !model) return VC_ERR_ARG;
    if (nmixtures < 1 || nmixtures > kMog2MaxMixtures)
        return fail(ctx, VC_ERR_ARG, "MOG2 with %d mixtures: this build keeps 1..%d per pixel", nmixtures, kMog2MaxMixtures);
    if (shadow_value < 0 || shadow_value > 255) return fail(ctx, VC_ERR_ARG, "MOG2 shadow value %d not in [0,255]", shadow_value);
    for (uint32_t i = 0; i < VC_MAX_MOG_MODELS; ++i) {
        vc_ctx::Mog2Model &m = ctx->mog2[i];
        if (m.used) continue;
        // the constructor (bgfg_gaussmix2.cpp, BackgroundSubtractorMOG2Impl): non-positive history / varThreshold select the defaults
        m.history = history > 0 ? history : 500;
        m.var_threshold = (double)(float)(var_threshold > 0 ? var_threshold : 16.0);
        m.shadows = detect_shadows != 0;
        m.nmixtures = nmixtures;
        m.background_ratio = (float)background_ratio;
        m.var_threshold_gen = (float)var_threshold_gen;
        m.var_init = (float)var_init; m.var_min = (float)var_min; m.var_max = (float)var_max;
        m.ct = (float)complexity_reduction_threshold;
        m.shadow_value = shadow_value;
        m.tau = (float)shadow_threshold;
        m.H = m.W = m.nframes = 0;
        m.used = true;
        *model = VC_MOG2_MODEL_TAG | i;
        return VC_OK;
    }
    return fail(ctx, VC_ERR_ARG, "all %d MOG2 background models of this context are in use", VC_MAX_MOG_MODELS);
}

int vc_mog2_destroy(vc_ctx *ctx, uint32_t model)
{
    if (!ctx) return VC_ERR_ARG;
    vc_ctx::Mog2Model *m = mog2_model(ctx, model);
    if (!m) return fail(ctx, VC_ERR_ARG, "no MOG2 background model %u", model);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
    m->state.reset();
    m->nmodes.reset();
    m->used = false;
    return VC_OK;
}

// One frame through a MOG2 model: d_img (device, [H W 3]) -> d_mask (device, [H W]) on the upload stream.
static int mog2_enqueue(vc_ctx *ctx, vc_ctx::Mog2Model &m, const uint8_t *d_img, uint32_t H, uint32_t W, double learning_rate, uint8_t *d_mask)
{
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    // apply(): the model starts over on its first frame, on a learning rate >= 1 and when the image size changes
    if (m.nframes == 0 || learning_rate >= 1 || m.H != H || m.W != W) {
        VC_TRY(ensure(ctx, m.state, npix * 5 * (size_t)m.nmixtures));
        VC_TRY(ensure(ctx, m.nmodes, npix));
        VC_HIP(ctx, hipMemsetAsync(m.state.ptr, 0, npix * 5 * (size_t)m.nmixtures * sizeof(float), st));
        VC_HIP(ctx, hipMemsetAsync(m.nmodes.ptr, 0, npix, st));
        m.H = H; m.W = W; m.nframes = 0;
    }
    ++m.nframes;
    const uint32_t two_n = 2 * m.nframes;
    const double lr = learning_rate >= 0 && m.nframes > 1 ? learning_rate : 1.0 / (double)(two_n < (uint32_t)m.history ? two_n : (uint32_t)m.history);
    Mog2Params p;
    p.alphaT = (float)lr; p.alpha1 = 1.f - p.alphaT; p.prune = (float)(-lr * (double)m.ct);
    p.Tb = (float)m.var_threshold; p.TB = m.background_ratio; p.Tg = m.var_threshold_gen;
    p.varInit = m.var_init; p.varMin = m.var_min; p.varMax = m.var_max; p.tau = m.tau;
    p.K = (uint32_t)m.nmixtures; p.npix = (uint32_t)npix; p.shadows = m.shadows ? 1u : 0u; p.shadowValue = (uint32_t)m.shadow_value;
    hipLaunchKernelGGL(k_mog2_apply, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, st, d_img, d_mask, m.state.ptr, m.nmodes.ptr, p);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

// Either kind of background model (checked by any_model).
static int model_enqueue(vc_ctx *ctx, uint32_t model, const uint8_t *d_img, uint32_t H, uint32_t W, double learning_rate, uint8_t *d_mask)
{
    if (vc_ctx::Mog2Model *m2 = mog2_model(ctx, model)) return mog2_enqueue(ctx, *m2, d_img, H, W, learning_rate, d_mask);
    return mog_enqueue(ctx, model, d_img, H, W, learning_rate, d_mask);
}

static int hsv_tables(vc_ctx *ctx)
{
    if (ctx->d_hsvdiv.ptr) return VC_OK;
    // as OpenCV builds them (color_hsv: RGB2HSV_b): saturate_cast<int>(double) = round half to even
    int32_t t[512];
    t[0] = t[256] = 0;
    for (int i = 1; i < 256; ++i) {
        t[i] = (int32_t)std::nearbyint((double)(255 << kHsvShift) / (1.0 * i));
        t[256 + i] = (int32_t)std::nearbyint((double)(180 << kHsvShift) / (6.0 * i));
    }
    VC_TRY(ensure(ctx, ctx->d_hsvdiv, 512));
    VC_HIP(ctx, hipMemcpy(ctx->d_hsvdiv.ptr, t, sizeof t, hipMemcpyHostToDevice));
    return VC_OK;
}

int vc_mog_apply(vc_ctx *ctx, uint32_t model, const uint8_t *image, uint32_t H, uint32_t W, double learning_rate, uint8_t *fgmask)
{
    if (!ctx || !image || !fgmask) return VC_ERR_ARG;
    if (model >= VC_MAX_MOG_MODELS || !ctx->mog[model].used) return fail(ctx, VC_ERR_ARG, "no background model %u", model);
    if (H == 0 || W == 0 || (uint64_t)H * W > 0x0fffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u", H, W);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(ensure(ctx, ctx->d_fg, npix * 6 + 64));
    uint8_t *d_in = ctx->d_fg.ptr, *d_out = d_in + npix * 3;
    VC_HIP(ctx, hipMemcpyAsync(d_in, image, npix * 3, hipMemcpyHostToDevice, st));
    VC_TRY(mog_enqueue(ctx, model, d_in, H, W, learning_rate, d_out));
    VC_HIP(ctx, hipMemcpyAsync(fgmask, d_out, npix, hipMemcpyDeviceToHost, st));
    VC_HIP(ctx, hipStreamSynchronize(st));
    return VC_OK;
}

int vc_mog2_apply(vc_ctx *ctx, uint32_t model, const uint8_t *image, uint32_t H, uint32_t W, double learning_rate, uint8_t *fgmask)
{
    if (!ctx || !image || !fgmask) return VC_ERR_ARG;
    vc_ctx::Mog2Model *m = mog2_model(ctx, model);
    if (!m) return fail(ctx, VC_ERR_ARG, "no MOG2 background model %u", model);
    if (H == 0 || W == 0 || (uint64_t)H * W > 0x0fffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u", H, W);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(ensure(ctx, ctx->d_fg, npix * 6 + 64));
    uint8_t *d_in = ctx->d_fg.ptr, *d_out = d_in + npix * 3;
    VC_HIP(ctx, hipMemcpyAsync(d_in, image, npix * 3, hipMemcpyHostToDevice, st));
    VC_TRY(mog2_enqueue(ctx, *m, d_in, H, W, learning_rate, d_out));
    VC_HIP(ctx, hipMemcpyAsync(fgmask, d_out, npix, hipMemcpyDeviceToHost, st));
    VC_HIP(ctx, hipStreamSynchronize(st));
    return VC_OK;
}

int vc_mog2_state(vc_ctx *ctx, uint32_t model, float *state, uint64_t capacity, uint8_t *nmodes, uint64_t nmodes_capacity, uint32_t *H,
                  uint32_t *W, uint32_t *nmixtures, uint32_t *nframes)
{
    if (!ctx) return VC_ERR_ARG;
    const vc_ctx::Mog2Model *m = mog2_model(ctx, model);
    if (!m) return fail(ctx, VC_ERR_ARG, "no MOG2 background model %u", model);
    if (H) *H = m->H;
    if (W) *W = m->W;
    if (nmixtures) *nmixtures = (uint32_t)m->nmixtures;
    if (nframes) *nframes = m->nframes;
    if (!state && !nmodes) return VC_OK;
    const size_t npix = (size_t)m->H * m->W, nfloat = npix * 5 * (size_t)m->nmixtures;
    if (state && capacity < nfloat)
        return fail(ctx, VC_ERR_ARG, "state buffer holds %llu floats, the model has %llu", (unsigned long long)capacity, (unsigned long long)nfloat);
    if (nmodes && nmodes_capacity < npix)
        return fail(ctx, VC_ERR_ARG, "nmodes buffer holds %llu bytes, the model has %llu pixels", (unsigned long long)nmodes_capacity, (unsigned long long)npix);
    if (npix == 0) return VC_OK;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
    if (state) VC_HIP(ctx, hipMemcpy(state, m->state.ptr, nfloat * sizeof(float), hipMemcpyDeviceToHost));
    if (nmodes) VC_HIP(ctx, hipMemcpy(nmodes, m->nmodes.ptr, npix, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_foreground_front(vc_ctx *ctx, uint32_t model, const uint8_t *bgr, uint32_t H, uint32_t W, int to_hsv, double learning_rate,
                        int open, int close, uint8_t *mask)
{
    if (!ctx || !bgr || !mask) return VC_ERR_ARG;
    if (!any_model(ctx, model)) return fail(ctx, VC_ERR_ARG, "no background model %u", model);
    if (H == 0 || W == 0 || (uint64_t)H * W > 0x0fffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u", H, W);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(hsv_tables(ctx));
    VC_TRY(ensure(ctx, ctx->d_fg, npix * 8 + 64));
    uint8_t *d_in = ctx->d_fg.ptr, *d_hsv = d_in + npix * 3, *a = d_hsv + npix * 3, *b = a + npix;
    VC_HIP(ctx, hipMemcpyAsync(d_in, bgr, npix * 3, hipMemcpyHostToDevice, st));
    const dim3 g((uint32_t)((npix + 255) / 256)), blk(256);
    if (to_hsv) {
        hipLaunchKernelGGL(k_bgr2hsv, g, blk, 0, st, (const uint8_t *)d_in, d_hsv, (uint32_t)npix, (const int32_t *)ctx->d_hsvdiv.ptr,
                           (const int32_t *)(ctx->d_hsvdiv.ptr + 256));
        VC_HIP(ctx, hipGetLastError());
    }
    VC_TRY(model_enqueue(ctx, model, to_hsv ? d_hsv : d_in, H, W, learning_rate, a));
    auto pass = [&](bool dilate) {
        if (dilate) hipLaunchKernelGGL(k_morph3x3<true>, g, blk, 0, st, (const uint8_t *)a, b, H, W);
        else hipLaunchKernelGGL(k_morph3x3<false>, g, blk, 0, st, (const uint8_t *)a, b, H, W);
        uint8_t *t = a; a = b; b = t;
    };
    if (open) { pass(false); pass(true); }
    if (close) { pass(true); pass(false); }
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(mask, a, npix, hipMemcpyDeviceToHost, st));
    VC_HIP(ctx, hipStreamSynchronize(st));
    return VC_OK;
}

// The contour stage (background_subtraction.py:171-193) of `cams` masks of H x W at d_mask ([cams][H W]) into d_out, on the
// upload stream; thresholds per camera.  Eight launches, the cameras in grid z, no host synchronisation (vc_contour.h).
static int fill_enqueue(vc_ctx *ctx, const uint8_t *d_mask, uint8_t *d_out, uint32_t H, uint32_t W, uint32_t cams, const double *T,
                        const double *t)
{
    if (cams == 0 || cams > kFillMaxCameras) return fail(ctx, VC_ERR_ARG, "contour stage of %u masks: 1..%u at once", cams, kFillMaxCameras);
    const uint64_t Np = (uint64_t)(H + 2) * (W + 2);
    if (Np >= 0x7fffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u too large for the contour stage", H, W);
    VC_TRY(ensure(ctx, ctx->d_cc, (size_t)Np * 4 * cams));
    FillParams p;
    memset(&p, 0, sizeof p);
    p.mask = d_mask; p.out = d_out;
    p.lab = ctx->d_cc.ptr;
    p.own = p.lab + (size_t)Np * cams;
    p.tot = p.own + (size_t)Np * cams;
    p.par = p.tot + (size_t)Np * cams;
    p.H = H; p.W = W; p.Wp = W + 2; p.Np = (uint32_t)Np;
    p.max_depth = (H < W ? H : W) + 4;
    for (uint32_t c = 0; c < cams; ++c) { p.T[c] = T[c]; p.t[c] = t[c]; }
    hipStream_t st = ctx->stream_up;
    const dim3 blk(kFillBlock);
    const dim3 gp((uint32_t)((Np + kFillBlock - 1) / kFillBlock), 1, cams);
    const dim3 gc((uint32_t)(((uint64_t)(H + 1) * (W + 1) + kFillBlock - 1) / kFillBlock), 1, cams);
    const dim3 gi((uint32_t)(((uint64_t)H * W + kFillBlock - 1) / kFillBlock), 1, cams);
    const dim3 gt((W + 2 + kTile - 1) / kTile, (H + 2 + kTile - 1) / kTile, cams);
    hipLaunchKernelGGL(k_fill_init, gp, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_local, gt, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_merge, gt, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_compress, gp, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_area, gc, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_subtree, gp, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_resolve, gp, blk, 0, st, p);
    hipLaunchKernelGGL(k_fill_output, gi, blk, 0, st, p);
    VC_HIP(ctx, hipGetLastError());
    return VC_OK;
}

int vc_fill_figures(vc_ctx *ctx, const uint8_t *mask, uint32_t H, uint32_t W, double figure_threshold, double inner_threshold, uint8_t *out)
{
    if (!ctx || !mask || !out) return VC_ERR_ARG;
    if (H == 0 || W == 0 || (uint64_t)H * W > 0x0fffffffull) return fail(ctx, VC_ERR_ARG, "image size %u x %u", H, W);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(ensure(ctx, ctx->d_fg, npix * 2 + 64));
    uint8_t *d_in = ctx->d_fg.ptr, *d_out = d_in + npix;
    VC_HIP(ctx, hipMemcpyAsync(d_in, mask, npix, hipMemcpyHostToDevice, st));
    VC_TRY(fill_enqueue(ctx, d_in, d_out, H, W, 1, &figure_threshold, &inner_threshold));
    VC_HIP(ctx, hipMemcpyAsync(out, d_out, npix, hipMemcpyDeviceToHost, st));
    VC_HIP(ctx, hipStreamSynchronize(st));
    return VC_OK;
}

int vc_foreground_to_slot(vc_ctx *ctx, uint32_t slot, const uint32_t *models, uint32_t n_models, const uint8_t *bgr, uint32_t H, uint32_t W,
                          double learning_rate, const double *figure_thr, const double *inner_thr, const uint8_t *open_pre,
                          const uint8_t *close_pre)
{
    if (!ctx || !models || !bgr || !figure_thr || !inner_thr) return VC_ERR_ARG;
    if (!ctx->have_cams) return fail(ctx, VC_ERR_ARG, "vc_set_cameras must precede vc_foreground_to_slot");
    const uint32_t C = ctx->C;
    if (n_models < C) return fail(ctx, VC_ERR_ARG, "vc_foreground_to_slot: %u background models for %u cameras", n_models, C);
    for (uint32_t c = 0; c < C; ++c)
        if (!any_model(ctx, models[c]))
            return fail(ctx, VC_ERR_ARG, "vc_foreground_to_slot: camera %u: no background model %u", c, models[c]);
    if (H != ctx->H || W != ctx->W)
        return fail(ctx, VC_ERR_ARG, "vc_foreground_to_slot: images of %u x %u, the cameras were set for %u x %u", H, W, ctx->H, ctx->W);
    if (slot >= 64) return fail(ctx, VC_ERR_ARG, "slot %u out of range (max 64 resident frame sets)", slot);
    Slot *s = nullptr;
    VC_TRY(slot_at(ctx, slot, &s));
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)H * W;
    hipStream_t st = ctx->stream_up;
    VC_TRY(hsv_tables(ctx));
    VC_TRY(ensure(ctx, s->bytes, HW * C + 64));
    VC_TRY(ensure(ctx, s->frames, HW * C));
    for (uint32_t c = 0; c < C; ++c) VC_TRY(ensure(ctx, s->fbytes[c], HW * 3 + 64));
    VC_TRY(ensure(ctx, s->bgr_all, HW * 3 * C));
    // scratch: HSV image | model mask | morphology buffer | the C pre-filtered masks
    VC_TRY(ensure(ctx, ctx->d_fg, HW * (5 + C) + 64));
    uint8_t *d_hsv = ctx->d_fg.ptr, *ma = d_hsv + HW * 3, *mb = ma + HW, *pre = mb + HW;
    VC_TRY(stage_upload(ctx, *s, s->h_bgr_all, s->bgr_all.ptr, bgr, HW * 3 * C, false));
    const dim3 g((uint32_t)((HW + 255) / 256)), blk(256);
    for (uint32_t c = 0; c < C; ++c) {
        const uint8_t *img = s->bgr_all.ptr + HW * 3 * c;
        VC_HIP(ctx, hipMemcpyAsync(s->fbytes[c].ptr, img, HW * 3, hipMemcpyDeviceToDevice, st));   // the records' colours
        hipLaunchKernelGGL(k_bgr2hsv, g, blk, 0, st, img, d_hsv, (uint32_t)HW, (const int32_t *)ctx->d_hsvdiv.ptr,
                           (const int32_t *)(ctx->d_hsvdiv.ptr + 256));
        uint8_t *a = ma, *b = mb;
        VC_TRY(model_enqueue(ctx, models[c], d_hsv, H, W, learning_rate, a));
        const bool op = open_pre && open_pre[c], cl = close_pre && close_pre[c];
        const int passes = (op ? 2 : 0) + (cl ? 2 : 0);
        int k = 0;
        auto pass = [&](bool dilate) {                           // a -> b (the last pass -> the camera's pre-filtered mask)
            uint8_t *dst = ++k == passes ? pre + HW * c : b;
            if (dilate) hipLaunchKernelGGL(k_morph3x3<true>, g, blk, 0, st, (const uint8_t *)a, dst, H, W);
            else hipLaunchKernelGGL(k_morph3x3<false>, g, blk, 0, st, (const uint8_t *)a, dst, H, W);
            b = a; a = dst;
        };
        if (op) { pass(false); pass(true); }
        if (cl) { pass(true); pass(false); }
        if (passes == 0) VC_HIP(ctx, hipMemcpyAsync(pre + HW * c, a, HW, hipMemcpyDeviceToDevice, st));
        VC_HIP(ctx, hipGetLastError());
    }
    VC_TRY(fill_enqueue(ctx, pre, s->bytes.ptr, H, W, C, figure_thr, inner_thr));
    s->have_masks = true;
    s->bits_valid = false;                                       // the next carve derives bits, images, grids from the new bytes
    s->grids_valid = false;
    for (uint32_t c = 0; c < C; ++c) { s->have_frame[c] = 1; s->frame_dirty[c] = 1; }
    return VC_OK;
}

int vc_mog_state(vc_ctx *ctx, uint32_t model, float *state, uint64_t capacity, uint32_t *H, uint32_t *W, uint32_t *nmixtures, uint32_t *nframes)
{
    if (!ctx) return VC_ERR_ARG;
    if (model >= VC_MAX_MOG_MODELS || !ctx->mog[model].used) return fail(ctx, VC_ERR_ARG, "no background model %u", model);
    const vc_ctx::MogModel &m = ctx->mog[model];
    if (H) *H = m.H;
    if (W) *W = m.W;
    if (nmixtures) *nmixtures = (uint32_t)m.nmixtures;
    if (nframes) *nframes = m.nframes;
    if (!state) return VC_OK;
    const size_t nfloat = (size_t)m.H * m.W * 8 * (size_t)m.nmixtures;
    if (capacity < nfloat) return fail(ctx, VC_ERR_ARG, "state buffer holds %llu floats, the model has %llu", (unsigned long long)capacity, (unsigned long long)nfloat);
    if (nfloat == 0) return VC_OK;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream_up));
    VC_HIP(ctx, hipMemcpy(state, m.state.ptr, nfloat * sizeof(float), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_set_option(vc_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name) return VC_ERR_ARG;
    const std::string k(name);
    if (k == "force_generic") ctx->force_generic = value != 0;
    else if (k == "reorder") ctx->reorder = value != 0;
    else if (k == "lut_hier") ctx->lut_hier = value != 0;
    else if (k == "fused_hier") ctx->fused_hier = value != 0;
    else if (k == "emit_lanes") ctx->emit_lanes = value != 0;
    else if (k == "overlap") ctx->overlap = value != 0;
    else if (k == "timing_detail") ctx->timing_detail = value != 0;
    else if (k == "kernel_events") ctx->kernel_events = value != 0;
    else if (k == "launch_events") ctx->launch_events = value != 0;
    else if (k == "event_scope" && value >= 0 && value <= 2) {
        if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
        VC_HIP(ctx, hipSetDevice(ctx->device));
        VC_TRY(vc_synchronize(ctx));
        ctx->event_scope = value;
        VC_HIP(ctx, make_events(ctx));
    }
    else if ((k == "stream_priority" && (value == 0 || value == 1)) || (k == "reserve_cus" && value >= 0 && value <= 16)) {
        if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
        VC_HIP(ctx, hipSetDevice(ctx->device));
        VC_TRY(vc_synchronize(ctx));
        (k == "stream_priority" ? ctx->stream_priority : ctx->reserve_cus) = value;
        VC_HIP(ctx, make_streams(ctx));
    }
    else if (k == "visible_check") ctx->visible.check = value != 0;
    else if (k == "visible_big_rect" && value >= 1) ctx->visible.big_rect = value;
    else if (k == "render_blocks") ctx->render.blocks = value != 0;
    else if (k == "surface_order") ctx->surface.order = value != 0;
    else if (k == "cluster_floor_records") ctx->clusters.floor_records = value != 0;
    else if (k == "geodesic_tiles") ctx->geodesic.tiles = value != 0;
    else if (k == "thin_table") ctx->thin.use_table = value != 0;
    else if (k == "cull") ctx->cull = value != 0;
    else if (k == "bricks") ctx->bricks = value != 0;
    else if (k == "dbg") ctx->dbg = value;
    else if (k == "voxel_pairs") ctx->voxel_pairs = value;
    else if (k == "voxel_batches" && value >= 0 && value <= 16) ctx->voxel_batches = value;
    else if (k == "emit_busy" && value >= 0 && value <= 2) ctx->emit_busy = value;          // 0 never, 1 large grids, 2 always
    else if (k == "emit_lut16") ctx->emit_lut16 = value != 0;                               // read by the next vc_carve_begin
    else if (k == "emit_waves_per_cu" && value >= 4 && value <= 1024) ctx->emit_waves_per_cu = value;
    else if (k == "lut_tile") ctx->lut_tile = value != 0;
    else if (k == "grid_lds_kb" && value >= 0 && value <= 148) ctx->grid_lds_kb = value;
    else if (k == "grid_min_shift" && value >= 0 && value <= 8) ctx->grid_min_shift = value;
    else if (k == "fused_tile") ctx->fused_tile = value != 0;
    else if (k == "fused_f32box") ctx->fused_f32box = value != 0;
    else if (k == "fused_boxes") ctx->fused_boxes = value != 0;
    else if (k == "fused_color_table") ctx->fused_color_table = value != 0;
    else if (k == "gather_compact") ctx->gather_compact = value != 0;
    else if (k == "gather_sync") ctx->gather_sync = value != 0;
    else if (k == "refine_pair") ctx->refine_pair = value != 0;
    else if (k == "hier_blocks_per_cu" && value >= 1 && value <= 4096) ctx->hier_blocks_per_cu = value;
    else if (k == "first_kv" && (value == 1 || value == 2 || value == 4)) ctx->first_kv = value;
    else if (k == "first_blocks_per_cu" && value >= 1 && value <= 8) ctx->first_blocks_per_cu = value;
    else if (k == "refine_b" && (value == 8 || value == 16)) ctx->refine_b = value;
    else if (k == "refine_blocks_per_cu" && value >= 1 && value <= 64) ctx->refine_blocks_per_cu = value;
    else if (k == "fused_blocks_per_cu" && value >= 1 && value <= 16) ctx->fused_blocks_per_cu = value;
    else return fail(ctx, VC_ERR_ARG, "unknown option or bad value: %s = %d", name, value);
    return VC_OK;
}

int vc_debug_counters(vc_ctx *ctx, uint64_t out[8])
{
    if (!ctx || !out) return VC_ERR_ARG;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memset(out, 0, 8 * sizeof(uint64_t));
    CarveParams p;
    fill_params(ctx, p);
    if (ctx->d_blist.ptr) {
        std::vector<uint32_t> c(6 * (size_t)kShards * kShardStride);
        VC_HIP(ctx, hipMemcpy(c.data(), ctx->d_blist.ptr, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        const uint32_t *q = c.data() + (size_t)ctx->list_parity * 3 * kShards * kShardStride;
        for (uint32_t k = 0; k < kShards; ++k) {
            out[0] += q[k * kShardStride]; out[4] += q[(kShards + k) * kShardStride]; out[5] += q[(2 * kShards + k) * kShardStride];
        }
    }
    if (ctx->d_live.ptr && ctx->kbox_valid) {
        const size_t nw = p.nbrick_pad / 64;
        std::vector<uint64_t> bits(2 * nw);
        VC_HIP(ctx, hipMemcpy(bits.data(), ctx->d_live.ptr, bits.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nw; ++i) { out[1] += (uint64_t)__builtin_popcountll(bits[i]); out[2] += (uint64_t)__builtin_popcountll(bits[nw + i]); }
        out[3] = (uint64_t)p.nbx * p.tq * p.nbz;
    }
    out[6] = ctx->last_emit16 ? 1 : 0;
    out[7] = ctx->lut16_cam >= 0 ? 1 : 0;
    return VC_OK;
}

int vc_timing(vc_ctx *ctx, vc_timing_t *out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    VC_TRY(finish_gather(ctx));
    if (ctx->h2d_pending && hipEventQuery(ctx->ev_h[1]) == hipSuccess) {
        (void)hipEventElapsedTime(&ctx->tm.h2d_ms, ctx->ev_h[0], ctx->ev_h[1]);
        ctx->h2d_pending = false;
    }
    memset(ctx->tm.work, 0, sizeof ctx->tm.work);
    if (ctx->d_stats.ptr && ctx->npending == 0) {
        std::vector<unsigned long long> h(ctx->d_stats.cap);
        VC_HIP(ctx, hipSetDevice(ctx->device));
        VC_HIP(ctx, hipMemcpy(h.data(), ctx->d_stats.ptr, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int w = 0; w < VC_WORK_KINDS; ++w)
            for (uint32_t k = 0; k < kShards; ++k) ctx->tm.work[w] += h[((size_t)w * kShards + k) * kStatStride];
    }
    ctx->tm.work[VC_WORK_DIST_CELLS] += ctx->distance.work[0];       // (counted on the host: the boxes are known there)
    ctx->tm.work[VC_WORK_DIST_LINES] += ctx->distance.work[1];
    *out = ctx->tm;
    return VC_OK;
}

uint32_t vc_timing_struct_size(void) { return (uint32_t)sizeof(vc_timing_t); }

int vc_timing_reset(vc_ctx *ctx)
{
    if (!ctx) return VC_ERR_ARG;
    ctx->tm.carve_launches = 0;
    ctx->tm.carve_ms_sum = 0;
    ctx->tm.first_ms_sum = 0;
    ctx->tm.gather_ms_sum = 0;
    ctx->tm.gathers = 0;
    ctx->tm.prep_ms_sum = 0;
    ctx->tm.preps = 0;
    ctx->tm.preps_timed = 0;
    ctx->tm.emit_ms_sum = 0;
    ctx->tm.emit_launches = 0;
    memset(ctx->tm.kernel_ms_sum, 0, sizeof ctx->tm.kernel_ms_sum);
    memset(ctx->tm.kernel_launches, 0, sizeof ctx->tm.kernel_launches);
    ctx->distance.work[0] = ctx->distance.work[1] = 0;
    if (ctx->d_stats.ptr && ctx->npending == 0) {
        VC_HIP(ctx, hipSetDevice(ctx->device));
        VC_HIP(ctx, hipMemset(ctx->d_stats.ptr, 0, ctx->d_stats.cap * sizeof(unsigned long long)));
    }
    return VC_OK;
}

// ---------------------------------------------------------------- multi-GPU
int vc_comm_unique_id(uint8_t out[VC_UNIQUE_ID_BYTES])
{
    if (!out) return VC_ERR_ARG;
    std::string err;
    if (!load_rccl(err)) return fail(nullptr, VC_ERR_RCCL, "%s", err.c_str());
    static_assert(sizeof(ncclUniqueId) == VC_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    VC_NCCL(nullptr, g_rccl.GetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return VC_OK;
}

int vc_comm_init(vc_ctx *ctx, int n_ranks, int rank, const uint8_t uid[VC_UNIQUE_ID_BYTES])
{
    if (!ctx || !uid) return VC_ERR_ARG;
    if (n_ranks < 1 || n_ranks > VC_MAX_RANKS || rank < 0 || rank >= n_ranks) return fail(ctx, VC_ERR_ARG, "rank %d of %d", rank, n_ranks);
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    std::string err;
    if (!load_rccl(err)) return fail(ctx, VC_ERR_RCCL, "%s", err.c_str());
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->comm) { g_rccl.CommDestroy(ctx->comm); ctx->comm = nullptr; }
    ncclUniqueId id;
    memcpy(&id, uid, sizeof id);
    VC_NCCL(ctx, g_rccl.CommInitRank(&ctx->comm, n_ranks, id, rank));
    ctx->n_ranks = n_ranks;
    ctx->rank = rank;
    VC_TRY(ensure(ctx, ctx->d_counts, (size_t)n_ranks + 1));
    VC_HIP(ctx, ensure_pinned(ctx->h_counts, (size_t)n_ranks));
    return VC_OK;
}

int vc_comm_destroy(vc_ctx *ctx)
{
    if (!ctx) return VC_ERR_ARG;
    if (ctx->comm) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipStreamSynchronize(ctx->stream_x);
        ctx->gpend[0] = ctx->gpend[1] = false;
        VC_NCCL(ctx, g_rccl.CommDestroy(ctx->comm));
        ctx->comm = nullptr;
    }
    ctx->n_ranks = 1; ctx->rank = 0;
    return VC_OK;
}

// ---- compact exchange form: the slab's non-zero occupancy words ----------------------------------
int vc_pack_entries(vc_ctx *ctx, uint64_t *n_entries_out)
{
    if (!ctx || !n_entries_out) return VC_ERR_ARG;
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "no carve result to pack");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(enqueue_pack(ctx, ctx->sb[ctx->cur], ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->packed_entries = *ctx->h_xtotal;
    ctx->packed = true;
    *n_entries_out = ctx->packed_entries;
    return VC_OK;
}

int vc_fetch_entries(vc_ctx *ctx, uint64_t *entries)
{
    if (!ctx || !entries) return VC_ERR_ARG;
    if (!ctx->packed) return fail(ctx, VC_ERR_ARG, "no packed result: call vc_pack_entries");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->packed_entries)
        VC_HIP(ctx, hipMemcpy(entries, ctx->sb[ctx->cur].ent.ptr, ctx->packed_entries * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_expand_entries(vc_ctx *ctx, const uint64_t *entries, uint64_t n_entries, uint64_t *total_out)
{
    if (!ctx || !total_out || (!entries && n_entries)) return VC_ERR_ARG;
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "vc_expand_entries colours like the last carve: run one first");
    if (n_entries > (1ull << 26)) return fail(ctx, VC_ERR_ARG, "%llu entries exceed a u32 grid", (unsigned long long)n_entries);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(finish_gather(ctx));
    ctx->gathered = false;
    VC_TRY(ensure_exchange_scratch(ctx, 1));
    VC_TRY(ensure(ctx, ctx->d_ent_all[0], (size_t)(2 * n_entries)));
    if (n_entries)
        VC_HIP(ctx, hipMemcpyAsync(ctx->d_ent_all[0].ptr, entries, n_entries * 2 * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    VC_TRY(enqueue_expand(ctx, ctx->stream, ctx->d_ent_all[0].ptr, n_entries, 0));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->gathered_total = n_entries ? *(ctx->h_xtotal + 1) : 0;
    ctx->gathered = true;
    *total_out = ctx->gathered_total;
    return VC_OK;
}

// Compact form of vc_allgather: every rank packs its non-zero words, the {bits, base} pairs are
// exchanged (~12x fewer bytes over xGMI than the records they stand for at 1024^3), and every rank
// expands all pairs itself -- colours from its own copy of the colour camera's table and frame.
static int allgather_compact(vc_ctx *ctx, uint64_t *counts_out, uint64_t *total_out)
{
    const int G = ctx->n_ranks;
    StepBuf &cur = ctx->sb[ctx->cur];
    hipStream_t sx = ctx->overlap ? ctx->stream_x : ctx->stream;    // every collective of the compact form is queued here
    const uint32_t half = ctx->gseq & 1u;
    VC_TRY(finish_one(ctx, half));                               // the gather before last owned this half; the last one may still run
    DevBuf<uint64_t> &ent_all = ctx->d_ent_all[half];
    Event *E = ctx->gx[ctx->gx_next];                       // this gather's own events: see vc_ctx::gx
    ctx->gx_idx[half] = ctx->gx_next;
    ctx->gx_next = (ctx->gx_next + 1) % kGatherRing;
    VC_HIP(ctx, hipEventRecord(E[0], sx));
    if (!cur.counts_exchanged) {                 // vc_carve_begin did not do it (records were kept)
        VC_TRY(enqueue_pack(ctx, cur, sx));
        VC_TRY(enqueue_counts_exchange(ctx, cur, sx));
        VC_HIP(ctx, hipStreamSynchronize(sx));
    }
    uint64_t M = 0, S = 0;
    for (int r = 0; r < G; ++r) { M += cur.h_counts[2 * r]; S += cur.h_counts[2 * r + 1]; }
    if (2 * M > ent_all.cap) VC_TRY(ensure(ctx, ent_all, (size_t)(2 * M + M / 4 + 1024)));
    VC_TRY(ensure(ctx, cur.ent, 2));
    VC_NCCL(ctx, g_rccl.GroupStart());
    uint64_t disp = 0;
    for (int r = 0; r < G; ++r) {
        const uint64_t cnt = cur.h_counts[2 * r];
        if (cnt) {
            ncclResult_t rc = g_rccl.Broadcast(cur.ent.ptr, ent_all.ptr + 2 * disp, 2 * cnt, ncclUint64, r,
                                               ctx->comm, sx);
            if (rc != ncclSuccess) {
                g_rccl.GroupEnd();
                return fail(ctx, VC_ERR_RCCL, "ncclBroadcast(root %d): %s", r, g_rccl.GetErrorString(rc));
            }
        }
        disp += cnt;
    }
    VC_NCCL(ctx, g_rccl.GroupEnd());
    VC_HIP(ctx, hipEventRecord(E[2], sx));
    // the expansion runs beside the next step's carve (second stream) when the call does not wait for it anyway
    hipStream_t xs = (ctx->overlap && !ctx->gather_sync) ? ctx->stream2 : sx;
    if (xs != sx) VC_HIP(ctx, hipStreamWaitEvent(xs, E[2], 0));
    if (S) VC_TRY(enqueue_expand(ctx, xs, ent_all.ptr, M, S, ctx->h_xtotal + 2 + half));
    VC_HIP(ctx, hipEventRecord(E[1], xs));
    if (S && cur.color_cam >= 0 && xs != ctx->stream) ctx->lut_color_reader = E[1];   // (it may read the colour table there: ensure_color_table)
    if (S && cur.color_cam >= 0) {          // the expansion reads the slot's bits / images beside the carve stream
        Slot &sl = ctx->slots[cur.slot];
        sl.e_emit = E[1];
        sl.emit_pending = true;
    }
    ctx->gpend[half] = true;
    ctx->gexpect[half] = S;
    ctx->gseq++;
    if (counts_out) for (int r = 0; r < G; ++r) counts_out[r] = cur.h_counts[2 * r + 1];
    ctx->gathered_total = S;
    ctx->gathered = true;
    *total_out = S;
    if (ctx->gather_sync) VC_TRY(finish_gather(ctx));
    return VC_OK;
}

// Variable-length all-gather in rank order.  Default (option "gather_compact" = 1): the compact form
// above.  With the option off: counts first (one u64 per rank), then one grouped broadcast of the
// 8-byte records per root straight into its displacement of the gathered buffer.
int vc_allgather(vc_ctx *ctx, uint64_t *counts_out, uint64_t *total_out)
{
    if (!ctx || !total_out) return VC_ERR_ARG;
    if (!ctx->comm) return fail(ctx, VC_ERR_ARG, "vc_comm_init must precede vc_allgather");
    if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "no carve result to gather");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const int G = ctx->n_ranks;
    if (ctx->gather_compact) return allgather_compact(ctx, counts_out, total_out);
    VC_TRY(finish_gather(ctx));
    if (ctx->sb[ctx->cur].no_records)
        return fail(ctx, VC_ERR_ARG, "last carve ran with VC_FLAG_NO_RECORDS: the record exchange needs records");
    hipStream_t sx = ctx->overlap ? ctx->stream_x : ctx->stream;      // (the exchange stream: every collective of the communicator is queued there)
    uint64_t *d_mine = ctx->d_counts.ptr + G;
    *ctx->h_total = ctx->survivors;
    VC_HIP(ctx, hipEventRecord(ctx->ev[0], sx));
    VC_HIP(ctx, hipMemcpyAsync(d_mine, ctx->h_total, sizeof(uint64_t), hipMemcpyHostToDevice, sx));
    VC_NCCL(ctx, g_rccl.AllGather(d_mine, ctx->d_counts.ptr, 1, ncclUint64, ctx->comm, sx));
    VC_HIP(ctx, hipMemcpyAsync(ctx->h_counts, ctx->d_counts.ptr, sizeof(uint64_t) * G, hipMemcpyDeviceToHost, sx));
    VC_HIP(ctx, hipStreamSynchronize(sx));
    uint64_t total = 0;
    for (int r = 0; r < G; ++r) total += ctx->h_counts[r];
    VC_TRY(ensure(ctx, ctx->d_gathered, (size_t)total));
    StepBuf &cur = ctx->sb[ctx->cur];
    if (!cur.records.ptr) VC_TRY(ensure(ctx, cur.records, 1024));
    VC_NCCL(ctx, g_rccl.GroupStart());
    uint64_t disp = 0;
    for (int r = 0; r < G; ++r) {
        const uint64_t cnt = ctx->h_counts[r];
        if (cnt) {
            ncclResult_t rc = g_rccl.Broadcast(cur.records.ptr, ctx->d_gathered.ptr + disp, cnt, ncclUint64, r,
                                               ctx->comm, sx);
            if (rc != ncclSuccess) {
                g_rccl.GroupEnd();
                return fail(ctx, VC_ERR_RCCL, "ncclBroadcast(root %d): %s", r, g_rccl.GetErrorString(rc));
            }
        }
        disp += cnt;
    }
    VC_NCCL(ctx, g_rccl.GroupEnd());
    VC_HIP(ctx, hipEventRecord(ctx->ev[1], sx));
    VC_HIP(ctx, hipStreamSynchronize(sx));
    VC_HIP(ctx, hipEventElapsedTime(&ctx->tm.gather_ms, ctx->ev[0], ctx->ev[1]));
    ctx->tm.exchange_ms = ctx->tm.gather_ms;
    ctx->tm.gather_ms_sum += ctx->tm.gather_ms;
    ctx->tm.gathers += 1;
    if (counts_out) memcpy(counts_out, ctx->h_counts, sizeof(uint64_t) * G);
    ctx->gathered_total = total;
    ctx->gathered = true;
    *total_out = total;
    return VC_OK;
}

// Max over ranks of one double, through the device (RCCL all-reduce): a barrier and a timing
// reduction for host code that must not load a second ROCm runtime.
int vc_comm_allreduce_max(vc_ctx *ctx, double *inout)
{
    if (!ctx || !inout) return VC_ERR_ARG;
    if (!ctx->comm) return fail(ctx, VC_ERR_ARG, "vc_comm_init must precede vc_comm_allreduce_max");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(ensure(ctx, ctx->d_scratch, 16));
    double *d = ctx->d_scratch.ptr;
    hipStream_t sx = ctx->overlap ? ctx->stream_x : ctx->stream;      // (every collective of the communicator on the one exchange stream)
    VC_HIP(ctx, hipMemcpyAsync(d, inout, sizeof(double), hipMemcpyHostToDevice, sx));
    VC_NCCL(ctx, g_rccl.AllReduce(d, d + 1, 1, ncclFloat64, ncclMax, ctx->comm, sx));
    VC_HIP(ctx, hipMemcpyAsync(inout, d + 1, sizeof(double), hipMemcpyDeviceToHost, sx));
    VC_HIP(ctx, hipStreamSynchronize(sx));
    return VC_OK;
}

int vc_fetch_gathered(vc_ctx *ctx, uint64_t *records)
{
    if (!ctx || !records) return VC_ERR_ARG;
    if (!ctx->gathered) return fail(ctx, VC_ERR_ARG, "no gathered result: call vc_allgather");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(finish_gather(ctx));
    if (ctx->gathered_total)
        VC_HIP(ctx, hipMemcpy(records, ctx->d_gathered.ptr, ctx->gathered_total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}
