// ---- coarse-to-fine block motion: vectors beyond the search range (vc_motion_pyramid.h; contract in include/voxcarve.h) ----
// Level 0 is motion.h's field in ctx->motion, so vc_fetch_motion, vc_hull_warp and vc_paint_motion read it as they read any field;
// the coarser levels live in ctx->pyramid.  Listing, ranking and the scan are motion.h's per level, with that level's grid.

// The grid of the next coarser level: ceil(n / 2) cells per axis, the same block edge, apron and search range.
static MotionGrid motion_coarser(const MotionGrid &f)
{
    MotionGrid g = f;
    g.nx = (f.nx + 1) / 2; g.ny = (f.ny + 1) / 2; g.nz = (f.nz + 1) / 2;
    g.nbx = (g.nx + g.b - 1) / g.b; g.nby = (g.ny + g.b - 1) / g.b; g.nbz = (g.nz + g.b - 1) / g.b;
    g.nblocks = g.nbx * g.nby * g.nbz;           // (at most the finer level's)
    g.n = (uint64_t)g.nx * g.ny * g.nz;
    g.nwords = (g.n + 63) / 64;
    return g;
}

int vc_hull_motion_pyramid(vc_ctx *ctx, uint32_t reg, uint32_t block, uint32_t apron, uint32_t search, uint32_t levels, uint32_t refine,
                           uint32_t flags, vc_motion_pyramid_stats_t *stats)
{
    static const char *const what = "vc_hull_motion_pyramid";
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "%s: stats must not be NULL", what);
    memset(stats, 0, sizeof *stats);
    Pass pass;
    VC_TRY(pass_open(ctx, what, "match", "motion", pass));
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "%s: flags must be 0 (got %u)", what, flags);
    VC_TRY(kept_refusals(ctx, what, reg, true));
    StepBuf &cur = *pass.cur;
    const uint64_t nwords = pass.nwords;
    MotionGrid g[kPyramidMaxLevels + 1];
    VC_TRY(motion_grid(ctx, what, block, apron, search, pass.n, nwords, g[0]));
    if (levels > kPyramidMaxLevels) return fail(ctx, VC_ERR_ARG, "%s: %u coarser levels, at most %u", what, levels, kPyramidMaxLevels);
    if (refine < 1 || refine > search) return fail(ctx, VC_ERR_ARG, "%s: refine radius %u not in 1..search = %u", what, refine, search);
    for (uint32_t l = 1; l <= levels; ++l) g[l] = motion_coarser(g[l - 1]);
    vc_ctx::Motion &M = ctx->motion;
    vc_ctx::Pyramid &P = ctx->pyramid;
    const vc_ctx::Kept &B = ctx->setops.reg[reg];
    if (B.words.cap < nwords) return fail(ctx, VC_ERR_INTERNAL, "%s: register %u holds %llu of %llu occupancy words", what, reg,
                                          (unsigned long long)B.words.cap, (unsigned long long)nwords);
    VC_TRY(pass_begin(ctx));
    M.stamp = kNever;
    VC_TRY(motion_sized(ctx, M, g[0]));          // (the scan's buffers with it: level 0 has the most groups)
    for (uint32_t l = 1; l <= levels; ++l) {
        VC_TRY(motion_sized(ctx, P.level[l - 1], g[l]));
        VC_TRY(ensure(ctx, P.wa[l - 1], (size_t)g[l].nwords));
        VC_TRY(ensure(ctx, P.wb[l - 1], (size_t)g[l].nwords));
    }
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    // the levels' words, A's and B's
    const uint64_t *wa[kPyramidMaxLevels + 1] = {cur.words.ptr}, *wb[kPyramidMaxLevels + 1] = {B.words.ptr};
    for (uint32_t l = 1; l <= levels; ++l) {
        for (int side = 0; side < 2; ++side) {
            MotionHalveParams hp;
            memset(&hp, 0, sizeof hp);
            hp.src = side ? wb[l - 1] : wa[l - 1];
            hp.dst = side ? P.wb[l - 1].ptr : P.wa[l - 1].ptr;
            hp.gs = g[l - 1]; hp.g = g[l];
            hipLaunchKernelGGL(k_motion_halve, dim3((uint32_t)((g[l].nwords + kMotionBlock - 1) / kMotionBlock)), dim3(kMotionBlock), 0, ctx->stream, hp);
            VC_HIP(ctx, hipGetLastError());
        }
        wa[l] = P.wa[l - 1].ptr; wb[l] = P.wb[l - 1].ptr;
    }
    // the coarsest level as vc_hull_motion matches, then every finer level around its parents' vectors; one read-back per level
    uint64_t listed[kPyramidMaxLevels + 1] = {0, 0, 0, 0};
    vc_ctx::Motion *lev[kPyramidMaxLevels + 1] = {&M, &P.level[0], &P.level[1], &P.level[2]};
    VC_TRY(motion_field(ctx, what, *lev[levels], g[levels], wa[levels], wb[levels], listed[levels]));
    for (uint32_t l = levels; l-- > 0;) {
        vc_ctx::Motion &F = *lev[l];
        VC_TRY(motion_listed(ctx, what, F, g[l], wa[l], wb[l], listed[l]));
        if (!listed[l]) continue;
        MotionRefineParams rp;
        memset(&rp, 0, sizeof rp);
        rp.a = wa[l]; rp.b = wb[l]; rp.g = g[l]; rp.r = refine;
        rp.rows = F.rows.ptr; rp.listed = listed[l]; rp.vec = F.vec.ptr;
        rp.pvec = lev[l + 1]->vec.ptr;
        rp.pnbx = g[l + 1].nbx; rp.pnby = g[l + 1].nby; rp.pnbz = g[l + 1].nbz; rp.pnblocks = g[l + 1].nblocks;
        rp.ctr = F.ctr.ptr;
        const uint32_t W = block + 2 * apron, R = W + 2 * refine;
        const size_t lds = ((size_t)R * R + (size_t)W * W) * sizeof(uint64_t);       // at most 51 200 bytes (refine <= search: R <= 64)
        hipLaunchKernelGGL(k_motion_refine, dim3((uint32_t)listed[l]), dim3(kMotionBlock), lds, ctx->stream, rp);
        VC_HIP(ctx, hipGetLastError());
    }
    VC_TRY(pass_stop(ctx, pass));
    for (uint32_t l = 0; l <= levels; ++l)
        VC_HIP(ctx, hipMemcpyAsync(lev[l]->h.ptr, lev[l]->ctr.ptr, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->motion_ms));
    uint64_t evaluated = 0;
    for (uint32_t l = 0; l <= levels; ++l) {
        const vc_ctx::Motion &F = *lev[l];
        if (motion_counters_bad(F, listed[l]))
            return fail(ctx, VC_ERR_HIP, "%s: level %u: %llu moved, %llu unique, %llu clipped of %llu listed blocks, cost %llu -> %llu", what, l,
                        (unsigned long long)F.h[0], (unsigned long long)F.h[1], (unsigned long long)F.h[2], (unsigned long long)listed[l],
                        (unsigned long long)F.h[3], (unsigned long long)F.h[4]);
        if (l == levels) continue;               // (the coarsest level has the five counters only)
        if (F.h[kPyramidOrphans] || F.h[kPyramidBorrowed] > listed[l])
            return fail(ctx, VC_ERR_HIP, "%s: level %u: %llu listed blocks without a listed parent, %llu of %llu borrowed", what, l,
                        (unsigned long long)F.h[kPyramidOrphans], (unsigned long long)F.h[kPyramidBorrowed], (unsigned long long)listed[l]);
        evaluated += F.h[kPyramidEvaluated];
    }
    const uint32_t reach = (search << levels) + refine * ((1u << levels) - 1u);      // at most 8 * 8 + 8 * 7 = 120
    stats->blocks = g[0].nblocks; stats->listed = listed[0]; stats->moved = M.h[0]; stats->unique = M.h[1]; stats->clipped = M.h[2];
    stats->cost0_sum = M.h[3]; stats->cost_sum = M.h[4]; stats->a = pass.S; stats->b = B.count;
    stats->levels = levels; stats->refine = refine; stats->reach = reach;
    for (uint32_t l = 0; l <= levels; ++l) {
        stats->listed_level[l] = listed[l];
        stats->dims_level[l][0] = g[l].nx; stats->dims_level[l][1] = g[l].ny; stats->dims_level[l][2] = g[l].nz;
    }
    stats->evaluated = evaluated;
    stats->borrowed = levels ? M.h[kPyramidBorrowed] : 0;
    for (uint32_t l = 0; l <= levels; ++l) { lev[l]->g = g[l]; lev[l]->listed = listed[l]; }
    M.reg = reg;
    M.levels = levels; M.refine = refine; M.reach = reach;
    M.stamp = ctx->result_gen;
    return VC_OK;
}

// The level of a fetch, refused when the current field has no such level.
static int motion_level(vc_ctx *ctx, const char *what, uint32_t level)
{
    VC_TRY(motion_current(ctx, what));
    if (level > ctx->motion.levels)
        return fail(ctx, VC_ERR_ARG, "%s: level %u, the field has the levels 0..%u", what, level, ctx->motion.levels);
    return VC_OK;
}

int vc_fetch_motion_level(vc_ctx *ctx, uint32_t level, vc_motion_t *rows, uint64_t *count)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(motion_level(ctx, "vc_fetch_motion_level", level));
    const vc_ctx::Motion &F = level ? ctx->pyramid.level[level - 1] : ctx->motion;
    if (count) *count = F.listed;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (rows && F.listed) VC_HIP(ctx, hipMemcpy(rows, F.rows.ptr, (size_t)F.listed * sizeof(vc_motion_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_motion_occupancy(vc_ctx *ctx, uint32_t level, uint32_t which, uint64_t *words, uint64_t *count)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(motion_level(ctx, "vc_fetch_motion_occupancy", level));
    if (which > 1) return fail(ctx, VC_ERR_ARG, "vc_fetch_motion_occupancy: which = %u, expected 0 (A) or 1 (B)", which);
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    const vc_ctx::Motion &M = ctx->motion;
    const vc_ctx::Motion &F = level ? ctx->pyramid.level[level - 1] : M;
    const uint64_t *src = nullptr;
    if (level) src = which ? ctx->pyramid.wb[level - 1].ptr : ctx->pyramid.wa[level - 1].ptr;
    else src = which ? ctx->setops.reg[M.reg].words.ptr : ctx->sb[ctx->cur].words.ptr;
    if (count) *count = F.g.nwords;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (words && F.g.nwords) {
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        VC_HIP(ctx, hipMemcpy(words, src, (size_t)F.g.nwords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return VC_OK;
}
