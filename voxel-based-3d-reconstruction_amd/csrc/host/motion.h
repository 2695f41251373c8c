// ---- block motion between a kept hull and the current result, its warp and its colours (vc_motion.h; contract in include/voxcarve.h) ----
constexpr uint64_t kMotionMaxBlocks = (uint64_t)kMaxScanBlocks * kScanBlock * 64u;   // a scan group is a wave of 64 blocks

// The parameters of a field as `what` refuses them, and the block grid of a result of n voxels in nwords words.
static int motion_grid(vc_ctx *ctx, const char *what, uint32_t block, uint32_t apron, uint32_t search, uint64_t n, uint64_t nwords, MotionGrid &g)
{
    if (block != 4 && block != 8 && block != 16) return fail(ctx, VC_ERR_ARG, "%s: block edge %u, expected 4, 8 or 16", what, block);
    if (apron > 16) return fail(ctx, VC_ERR_ARG, "%s: apron %u not in 0..16", what, apron);
    if (search < 1 || search > 8) return fail(ctx, VC_ERR_ARG, "%s: search range %u not in 1..8", what, search);
    if (block + 2 * apron + 2 * search > 64)
        return fail(ctx, VC_ERR_ARG, "%s: block + 2 apron + 2 search = %u exceeds the 64 bits of a row", what, block + 2 * apron + 2 * search);
    VC_TRY(merge_refuse_index(ctx, what, n));
    memset(&g, 0, sizeof g);
    g.nx = ctx->nx; g.ny = ctx->ny; g.nz = ctx->nz;
    g.nbx = (g.nx + block - 1) / block; g.nby = (g.ny + block - 1) / block; g.nbz = (g.nz + block - 1) / block;
    const uint64_t nblocks = (uint64_t)g.nbx * g.nby * g.nbz;
    if (!n || !nblocks || nblocks > kMotionMaxBlocks)
        return fail(ctx, VC_ERR_ARG, "%s: %llu blocks of edge %u, at most %llu", what, (unsigned long long)nblocks, block,
                    (unsigned long long)kMotionMaxBlocks);
    g.nblocks = (uint32_t)nblocks; g.b = block; g.a = apron; g.s = search; g.nwords = nwords; g.n = n;
    return VC_OK;
}

// The buffers of a field over g, all but the rows (which the listed blocks size, in the middle of motion_field).
static int motion_sized(vc_ctx *ctx, vc_ctx::Motion &M, const MotionGrid &g)
{
    const uint32_t ngroups = (g.nblocks + 63) / 64;
    VC_TRY(ensure(ctx, M.counts, (size_t)g.nblocks));
    VC_TRY(ensure(ctx, M.vec, (size_t)g.nblocks));
    VC_TRY(ensure(ctx, M.mask, ngroups));
    VC_TRY(ensure(ctx, M.ctr, 8));
    VC_TRY(ensure(ctx, ctx->d_rscan, ngroups));
    VC_HIP(ctx, ensure_pinned(M.h, 8));
    return VC_OK;
}

// The listed blocks of A and B over g into M: counters and vec zeroed, the rows with block, count_a and count_b at their ranks.
// Synchronous: the listed blocks are read back in the middle, they size the rows and the matching launch.
static int motion_listed(vc_ctx *ctx, const char *what, vc_ctx::Motion &M, const MotionGrid &g, const uint64_t *a, const uint64_t *b, uint64_t &listed)
{
    const uint64_t nblocks = g.nblocks;
    const uint32_t ngroups = (uint32_t)((nblocks + 63) / 64);
    VC_HIP(ctx, hipMemsetAsync(M.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(M.vec.ptr, 0, (size_t)nblocks * sizeof(uint32_t), ctx->stream));
    MotionListParams lp;
    memset(&lp, 0, sizeof lp);
    lp.a = a; lp.b = b; lp.g = g; lp.ngroups = ngroups;
    lp.counts = M.counts.ptr; lp.mask = M.mask.ptr; lp.cnt = ctx->d_rscan.cnt.ptr;
    hipLaunchKernelGGL(k_motion_list, dim3((ngroups + kMotionBlock / 64 - 1) / (kMotionBlock / 64)), dim3(kMotionBlock), 0, ctx->stream, lp);
    VC_HIP(ctx, hipGetLastError());
    // the read-back in the middle: the listed blocks size the rows and the matching launch
    VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_rscan, ctx->d_rscan.cnt.ptr, ngroups, ctx->h_res + 0));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    listed = ctx->h_res[0];
    if (listed > nblocks) return fail(ctx, VC_ERR_HIP, "%s: %llu of %llu blocks listed", what, (unsigned long long)listed, (unsigned long long)nblocks);
    VC_TRY(ensure(ctx, M.rows, (size_t)listed));
    if (listed) {
        hipLaunchKernelGGL(k_motion_rank, dim3((uint32_t)((nblocks + kMotionBlock - 1) / kMotionBlock)), dim3(kMotionBlock), 0, ctx->stream, g, ngroups,
                           (const uint32_t *)M.counts.ptr, (const uint64_t *)M.mask.ptr, (const uint32_t *)ctx->d_rscan.off.ptr,
                           (const uint64_t *)ctx->d_rscan.boff.ptr, M.rows.ptr, listed);
        VC_HIP(ctx, hipGetLastError());
    }
    return VC_OK;
}

// The field from B's words to A's into M (vec, rows, counters on the device), for vc_hull_motion, vc_hull_temporal_motion and the
// coarsest level of vc_hull_motion_pyramid.
static int motion_field(vc_ctx *ctx, const char *what, vc_ctx::Motion &M, const MotionGrid &g, const uint64_t *a, const uint64_t *b, uint64_t &listed)
{
    VC_TRY(motion_listed(ctx, what, M, g, a, b, listed));
    if (listed) {
        MotionMatchParams mp;
        memset(&mp, 0, sizeof mp);
        mp.a = a; mp.b = b; mp.g = g; mp.rows = M.rows.ptr; mp.listed = listed; mp.vec = M.vec.ptr; mp.ctr = M.ctr.ptr;
        const uint32_t W = g.b + 2 * g.a, R = W + 2 * g.s;
        const size_t lds = ((size_t)R * R + (size_t)W * W) * sizeof(uint64_t);       // at most 51 200 bytes (16 / 16 / 8: R = 64, W = 48)
        hipLaunchKernelGGL(k_motion_match, dim3((uint32_t)listed), dim3(kMotionBlock), lds, ctx->stream, mp);
        VC_HIP(ctx, hipGetLastError());
    }
    return VC_OK;
}

// The counters of motion_field once they are on the host (M.h): what cannot be.
static bool motion_counters_bad(const vc_ctx::Motion &M, uint64_t listed)
{
    return M.h[0] > listed || M.h[1] > listed || M.h[2] > listed || M.h[4] > M.h[3];
}

int vc_hull_motion(vc_ctx *ctx, uint32_t reg, uint32_t block, uint32_t apron, uint32_t search, uint32_t flags, vc_motion_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_motion: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_motion", "match", "motion", pass));
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_motion: flags must be 0 (got %u)", flags);
    VC_TRY(kept_refusals(ctx, "vc_hull_motion", reg, true));
    StepBuf &cur = *pass.cur;
    const uint64_t nwords = pass.nwords;
    MotionGrid g;
    VC_TRY(motion_grid(ctx, "vc_hull_motion", block, apron, search, pass.n, nwords, g));
    vc_ctx::Motion &M = ctx->motion;
    const vc_ctx::Kept &B = ctx->setops.reg[reg];
    if (B.words.cap < nwords) return fail(ctx, VC_ERR_INTERNAL, "vc_hull_motion: register %u holds %llu of %llu occupancy words", reg,
                                          (unsigned long long)B.words.cap, (unsigned long long)nwords);
    VC_TRY(pass_begin(ctx));
    M.stamp = kNever;
    VC_TRY(motion_sized(ctx, M, g));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    uint64_t listed = 0;
    VC_TRY(motion_field(ctx, "vc_hull_motion", M, g, cur.words.ptr, B.words.ptr, listed));
    VC_TRY(pass_stop(ctx, pass));
    VC_HIP(ctx, hipMemcpyAsync(M.h.ptr, M.ctr.ptr, kMotionCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->motion_ms));
    if (motion_counters_bad(M, listed))
        return fail(ctx, VC_ERR_HIP, "vc_hull_motion: %llu moved, %llu unique, %llu clipped of %llu listed blocks, cost %llu -> %llu", (unsigned long long)M.h[0],
                    (unsigned long long)M.h[1], (unsigned long long)M.h[2], (unsigned long long)listed, (unsigned long long)M.h[3], (unsigned long long)M.h[4]);
    stats->blocks = g.nblocks; stats->listed = listed; stats->moved = M.h[0]; stats->unique = M.h[1]; stats->clipped = M.h[2];
    stats->cost0_sum = M.h[3]; stats->cost_sum = M.h[4]; stats->a = pass.S; stats->b = B.count;
    M.g = g; M.listed = listed; M.reg = reg;
    M.levels = 0; M.refine = 0; M.reach = search;
    M.stamp = ctx->result_gen;
    return VC_OK;
}

// The field of the last vc_hull_motion is current: made on this result, against a register nobody has written since.
static int motion_current(vc_ctx *ctx, const char *what)
{
    if (!ctx->carved || !ctx->current(ctx->motion.stamp))
        return fail(ctx, VC_ERR_ARG, "%s: no motion field: call vc_hull_motion on the current carve result", what);
    return VC_OK;
}

int vc_fetch_motion(vc_ctx *ctx, vc_motion_t *rows, uint64_t *count)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(motion_current(ctx, "vc_fetch_motion"));
    static_assert(sizeof(vc_motion_t) == sizeof(MotionRow), "vc_motion_t");
    if (count) *count = ctx->motion.listed;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (rows && ctx->motion.listed)
        VC_HIP(ctx, hipMemcpy(rows, ctx->motion.rows.ptr, (size_t)ctx->motion.listed * sizeof(vc_motion_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_hull_warp(vc_ctx *ctx, uint32_t src, uint32_t dst, uint32_t flags, vc_warp_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_warp: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_warp", "warp", "motion", pass));
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_warp: flags must be 0 (got %u)", flags);
    VC_TRY(kept_refusals(ctx, "vc_hull_warp", src, true));
    VC_TRY(kept_refusals(ctx, "vc_hull_warp", dst, false));
    if (src == dst) return fail(ctx, VC_ERR_ARG, "vc_hull_warp: source and target are both register %u", src);
    VC_TRY(motion_current(ctx, "vc_hull_warp"));
    vc_ctx::Motion &M = ctx->motion;
    if (M.reg != src) return fail(ctx, VC_ERR_ARG, "vc_hull_warp: the motion field was made against register %u, not %u", M.reg, src);
    StepBuf &cur = *pass.cur;
    const uint64_t n = pass.n, nwords = pass.nwords, npad = (nwords + 1) & ~1ull;
    VC_TRY(merge_refuse_index(ctx, "vc_hull_warp", n));
    const vc_ctx::Kept &B = ctx->setops.reg[src];
    if (M.g.n != n || M.g.nwords != nwords || B.words.cap < nwords)
        return fail(ctx, VC_ERR_INTERNAL, "vc_hull_warp: the field's grid of %llu voxels is not the result's %llu", (unsigned long long)M.g.n, (unsigned long long)n);
    VC_TRY(pass_begin(ctx));
    vc_ctx::Kept k;                              // built beside the register, which stays as it is until the prediction is whole
    VC_TRY(ensure(ctx, k.words, (size_t)npad));
    VC_TRY(ensure(ctx, M.ctr, 8));
    VC_HIP(ctx, ensure_pinned(M.h, 8));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    VC_HIP(ctx, hipMemsetAsync(M.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    MotionWarpParams wp;
    memset(&wp, 0, sizeof wp);
    wp.a = cur.words.ptr; wp.b = B.words.ptr; wp.g = M.g; wp.vec = M.vec.ptr; wp.out = k.words.ptr; wp.npad = npad; wp.ctr = M.ctr.ptr;
    hipLaunchKernelGGL(k_motion_warp, dim3((uint32_t)((npad + kSetopBlock - 1) / kSetopBlock)), dim3(kSetopBlock), 0, ctx->stream, wp);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(pass_stop(ctx, pass));
    VC_HIP(ctx, hipMemcpyAsync(M.h.ptr, M.ctr.ptr, kWarpCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->warp_ms));
    if (M.h[0] > n || M.h[1] > M.h[0] || M.h[1] > pass.S)
        return fail(ctx, VC_ERR_HIP, "vc_hull_warp: %llu predicted voxels, %llu of them among %llu survivors", (unsigned long long)M.h[0],
                    (unsigned long long)M.h[1], (unsigned long long)pass.S);
    stats->warped = M.h[0]; stats->common = M.h[1]; stats->a = pass.S;
    k.count = M.h[0]; k.used = true; k.has_rec = false;
    ctx->setops.reg[dst] = std::move(k);
    return VC_OK;
}

int vc_paint_motion(vc_ctx *ctx)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(motion_current(ctx, "vc_paint_motion"));
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->survivors) return VC_OK;
    StepBuf &cur = ctx->sb[ctx->cur];
    VC_HIP(ctx, hipSetDevice(ctx->device));
    MotionGrid g = ctx->motion.g;
    g.s = ctx->motion.reach;                     // the largest component a vector of the field can have (vc_hull_motion: the search range)
    hipLaunchKernelGGL(k_motion_paint, dim3((uint32_t)((ctx->survivors + kMotionBlock - 1) / kMotionBlock)), dim3(kMotionBlock), 0, ctx->stream,
                       cur.records.ptr, ctx->survivors, g, (const uint32_t *)ctx->motion.vec.ptr);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VC_OK;
}
