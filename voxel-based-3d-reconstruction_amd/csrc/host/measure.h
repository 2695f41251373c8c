// ---- the hull's figures measured per group of records (vc_measure.h; contract in include/voxcarve.h) ----
static_assert(sizeof(vc_measure_t) == kMsStride * sizeof(uint64_t) && offsetof(vc_measure_t, lo) == kMsSums * sizeof(uint64_t),
              "the kernels lay an entry out as vc_measure_t");

static MsDiv ms_divisor(uint32_t d)
{
    MsDiv q;
    q.m = (unsigned long long)(0xffffffffffffffffull / d + 1ull);    // (d = 1 wraps to 0: ms_div takes that for "by one")
    q.d = d;
    return q;
}

#define VC_MS_FOLD()                                                                                                                    \
    hipLaunchKernelGGL(k_ms_fold, dim3((p.tab * kMsStride * kMsFoldSlices + kMsBlock - 1) / kMsBlock), dim3(kMsBlock), 0, ctx->stream,  \
                       (const unsigned long long *)p.part, grid.x, p.tab * kMsStride, p.out)
// The launches of one label form (kMsLabels*): the sums per group, then the profile if asked for.
#define VC_MS_LAUNCH(KIND)                                                                                                              \
    do {                                                                                                                                \
        hipLaunchKernelGGL(k_ms_groups<KIND>, grid, dim3(kMsBlock), (size_t)p.tab * kMsStride * sizeof(uint64_t), ctx->stream, p);      \
        VC_MS_FOLD();                                                                                                                   \
        if (profile) hipLaunchKernelGGL(k_ms_profile<KIND>, grid, dim3(kMsBlock), 0, ctx->stream, p);                                   \
    } while (0)

int vc_hull_measure(vc_ctx *ctx, uint32_t source, const uint32_t *labels, uint32_t groups, uint32_t flags, vc_measure_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_measure: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags & ~VC_MEASURE_PROFILE) return fail(ctx, VC_ERR_ARG, "vc_hull_measure: unknown flags %u (VC_MEASURE_PROFILE)", flags);
    if (source > VC_MEASURE_HOST)
        return fail(ctx, VC_ERR_ARG, "vc_hull_measure: source %u, expected 0 (all), 1 (clusters), 2 (geodesic) or 3 (host labels)", source);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_measure", "measure", "measuring", pass));
    const uint64_t S = pass.S, n = pass.n, nwords = pass.nwords;
    if (ctx->nx > VC_MEASURE_MAX_AXIS || ctx->ny > VC_MEASURE_MAX_AXIS || ctx->nz > VC_MEASURE_MAX_AXIS)
        return fail(ctx, VC_ERR_ARG, "vc_hull_measure: the grid %u x %u x %u has an axis of more than %u cells", ctx->nx, ctx->ny, ctx->nz,
                    VC_MEASURE_MAX_AXIS);
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_measure: %llu voxels exceed the u32 index", (unsigned long long)n);
    uint32_t G = 1;
    const void *dev_labels = nullptr;
    if (source == VC_MEASURE_CLUSTERS) {
        if (!ctx->current(ctx->clusters.stamp))
            return fail(ctx, VC_ERR_ARG, "vc_hull_measure: no clusters of the current carve result to take the labels from: call vc_hull_clusters first");
        G = ctx->clusters.k;
        dev_labels = ctx->clusters.lab.ptr;
    } else if (source == VC_MEASURE_GEODESIC) {
        if (!ctx->current(ctx->geodesic.stamp))
            return fail(ctx, VC_ERR_ARG, "vc_hull_measure: no geodesic regions of the current carve result to take the labels from: call vc_hull_geodesic first");
        G = (uint32_t)ctx->geodesic.ext.size() + 1u;
        dev_labels = ctx->geodesic.key.ptr;
    } else if (source == VC_MEASURE_HOST) {
        if (!labels) return fail(ctx, VC_ERR_ARG, "vc_hull_measure: VC_MEASURE_HOST and no labels");
        G = groups;
    }
    if (G < 1 || G > VC_MEASURE_MAX_GROUPS) return fail(ctx, VC_ERR_ARG, "vc_hull_measure: G = %u not in [1, %u]", G, VC_MEASURE_MAX_GROUPS);
    const bool profile = (flags & VC_MEASURE_PROFILE) != 0;
    if (profile && (uint64_t)G * ctx->nz > VC_MEASURE_MAX_PROFILE)
        return fail(ctx, VC_ERR_ARG, "vc_hull_measure: a profile of %u groups x %u layers exceeds %u entries", G, ctx->nz, VC_MEASURE_MAX_PROFILE);
    if (source == VC_MEASURE_HOST)
        for (uint64_t s = 0; s < S; ++s)
            if (labels[s] >= G && labels[s] != 0xffffffffu)
                return fail(ctx, VC_ERR_ARG, "vc_hull_measure: record %llu has label %u, not below G = %u and not 0xffffffff", (unsigned long long)s,
                            labels[s], G);
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->measure.stamp = kNever;
    const size_t cells = (size_t)G * kMsStride, pcells = profile ? (size_t)G * ctx->nz * 3 : 0;
    VC_HIP(ctx, ensure_pinned(ctx->measure.h, cells));
    VC_TRY(ensure(ctx, ctx->measure.out, cells));
    if (profile) VC_TRY(ensure(ctx, ctx->measure.prof, pcells));
    if (source == VC_MEASURE_HOST && S) VC_TRY(ensure(ctx, ctx->measure.lab, (size_t)S));
    // as many workgroups as their tables fit kMsPartBytes, between a workgroup per compute unit and kMsMaxBlocks
    const uint32_t tab = source == VC_MEASURE_ALL ? 1u : G < kMsTable ? G : kMsTable;
    uint64_t most = kMsPartBytes / ((uint64_t)tab * kMsStride * sizeof(uint64_t));
    most = most > kMsMaxBlocks ? kMsMaxBlocks : most < 256 ? 256 : most;
    uint64_t blocks = (S + kMsBlock - 1) / kMsBlock;
    if (blocks > most) blocks = most;
    const uint64_t per = S ? ((S + blocks - 1) / blocks + kMsBlock - 1) / kMsBlock * kMsBlock : kMsBlock;
    const dim3 grid((uint32_t)((S + per - 1) / per));
    if (S) VC_TRY(ensure(ctx, ctx->measure.part, (size_t)grid.x * tab * kMsStride));
    VC_TRY(pass_start(ctx, pass));
    hipLaunchKernelGGL(k_ms_init, dim3((uint32_t)((cells + kMsBlock - 1) / kMsBlock)), dim3(kMsBlock), 0, ctx->stream, ctx->measure.out.ptr, G);
    VC_HIP(ctx, hipGetLastError());
    if (profile) VC_HIP(ctx, hipMemsetAsync(ctx->measure.prof.ptr, 0, pcells * sizeof(uint64_t), ctx->stream));
    if (S) {
        if (source == VC_MEASURE_HOST) {
            VC_HIP(ctx, hipMemcpyAsync(ctx->measure.lab.ptr, labels, (size_t)S * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
            dev_labels = ctx->measure.lab.ptr;
        }
        MsParams p;
        memset(&p, 0, sizeof p);
        p.records = cur.records.ptr; p.words32 = reinterpret_cast<const uint32_t *>(cur.words.ptr); p.labels = dev_labels;
        p.out = ctx->measure.out.ptr; p.prof = profile ? ctx->measure.prof.ptr : nullptr;
        p.S = S; p.nw32 = 2 * nwords;
        p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz; p.ncol = ctx->nx * ctx->ny; p.G = G; p.tab = tab; p.per = per;
        p.by_ncol = ms_divisor(p.ncol); p.by_ny = ms_divisor(p.ny);
        p.part = ctx->measure.part.ptr;
        if (source == VC_MEASURE_ALL) {
            hipLaunchKernelGGL(k_ms_all, grid, dim3(kMsBlock), 0, ctx->stream, p);
            VC_MS_FOLD();
            if (profile) hipLaunchKernelGGL(k_ms_profile<kMsLabelsNone>, grid, dim3(kMsBlock), 0, ctx->stream, p);
        } else if (source == VC_MEASURE_CLUSTERS) VC_MS_LAUNCH(kMsLabelsU8);
        else if (source == VC_MEASURE_GEODESIC) VC_MS_LAUNCH(kMsLabelsKey);
        else VC_MS_LAUNCH(kMsLabelsU32);
        VC_HIP(ctx, hipGetLastError());
    }
    VC_HIP(ctx, hipMemcpyAsync(ctx->measure.h, ctx->measure.out.ptr, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->measure_ms));
    uint64_t measured = 0;
    for (uint32_t g = 0; g < G; ++g) measured += ctx->measure.h[(size_t)g * kMsStride + kMsVoxels];
    if (measured > S) return fail(ctx, VC_ERR_HIP, "vc_hull_measure: %llu records measured of %llu", (unsigned long long)measured, (unsigned long long)S);
    stats->survivors = S; stats->groups = G; stats->measured = measured; stats->unlabelled = S - measured;
    ctx->measure.g = G; ctx->measure.nz = ctx->nz; ctx->measure.profile = profile;
    ctx->measure.stamp = ctx->result_gen;
    return VC_OK;
}

// The refusal the two fetch calls share.
static int measure_current(vc_ctx *ctx)
{
    if (!ctx->carved || !ctx->current(ctx->measure.stamp)) return fail(ctx, VC_ERR_ARG, "no measurements: call vc_hull_measure on the current carve result");
    return VC_OK;
}

int vc_fetch_measure(vc_ctx *ctx, vc_measure_t *out)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(measure_current(ctx));
    if (!out) return VC_OK;                      // only asked whether the measurements are valid
    memcpy(out, ctx->measure.h, (size_t)ctx->measure.g * sizeof(vc_measure_t));
    return VC_OK;
}

int vc_fetch_measure_profile(vc_ctx *ctx, uint64_t *out)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(measure_current(ctx));
    if (!ctx->measure.profile) return fail(ctx, VC_ERR_ARG, "no measurements by layer: the last vc_hull_measure ran without VC_MEASURE_PROFILE");
    if (!out) return VC_OK;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipMemcpy(out, ctx->measure.prof.ptr, (size_t)ctx->measure.g * ctx->measure.nz * 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}
