// ---- the hull thinned to a curve skeleton (vc_thin.h; contract in include/voxcarve.h) ----
static_assert(sizeof(vc_skeleton_voxel_t) == sizeof(ThRow) && offsetof(vc_skeleton_voxel_t, degree) == 8, "k_thin_rows lays a row out as vc_skeleton_voxel_t");

// The predicate's table on the device, built once per context (on the context's stream: a launch behind it may read it).
static int thin_table(vc_ctx *ctx, uint32_t *launches)
{
    if (ctx->thin.table_built) return VC_OK;
    VC_TRY(ensure(ctx, ctx->thin.table, (size_t)kThTableWords));
    VC_DLAUNCH(kThinKind, k_thin_table, dim3(kThTableWords / kThBlock), dim3(kThBlock), ctx->thin.table.ptr);
    VC_HIP(ctx, hipGetLastError());
    if (launches) *launches += 1;
    ctx->thin.table_built = true;
    return VC_OK;
}

int vc_hull_thin(vc_ctx *ctx, uint32_t mode, uint32_t anchor_source, const uint32_t *anchors, uint64_t n_anchors, uint32_t max_passes,
                 uint32_t flags, vc_thin_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: unknown flags %u (none is defined)", flags);
    if (mode > VC_THIN_POINT) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: mode %u, expected 0 (curve) or 1 (point)", mode);
    if (anchor_source > VC_THIN_ANCHORS_EXTREMA)
        return fail(ctx, VC_ERR_ARG, "vc_hull_thin: anchor source %u, expected 0 (none), 1 (list) or 2 (extrema)", anchor_source);
    if (max_passes < 1 || max_passes > VC_THIN_MAX_PASSES)
        return fail(ctx, VC_ERR_ARG, "vc_hull_thin: max_passes = %u not in [1, %u]", max_passes, VC_THIN_MAX_PASSES);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_thin", "thin", "thinning", pass));
    const uint64_t S = pass.S, n = pass.n, nwords = pass.nwords;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: %llu voxels exceed the u32 index", (unsigned long long)n);
    if (anchor_source != VC_THIN_ANCHORS_LIST) n_anchors = 0;
    if (n_anchors && !anchors) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: %llu anchors and no list", (unsigned long long)n_anchors);
    if (n_anchors > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: %llu anchors exceed the u32 index", (unsigned long long)n_anchors);
    if (anchor_source == VC_THIN_ANCHORS_EXTREMA && !ctx->current(ctx->geodesic.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_hull_thin: no geodesic pass of the current carve result to take the anchors from: call vc_hull_geodesic first");
    if (!S && n_anchors) return fail(ctx, VC_ERR_ARG, "vc_hull_thin: anchor 0 (voxel %u) is no survivor", anchors[0]);
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    vc_ctx::Thin &T = ctx->thin;
    T.stamp = kNever;
    VC_HIP(ctx, ensure_pinned(T.h, kThCnt));
    memset(T.h, 0, kThCnt * sizeof(uint32_t));
    if (S) {
        VC_TRY(ensure(ctx, T.work, (size_t)nwords));
        VC_TRY(ensure(ctx, T.anchor, (size_t)nwords));
        VC_TRY(ensure(ctx, T.listed, (size_t)nwords));
        VC_TRY(ensure(ctx, T.woff, (size_t)nwords));
        VC_TRY(ensure(ctx, ctx->d_rscan, word_groups(nwords)));
        VC_TRY(ensure(ctx, T.live[0], (size_t)S));
        VC_TRY(ensure(ctx, T.live[1], (size_t)S));
        VC_TRY(ensure(ctx, T.cand, (size_t)S));
        VC_TRY(ensure(ctx, T.peel, (size_t)S));
        VC_TRY(ensure(ctx, T.rows, (size_t)S));
        VC_TRY(ensure(ctx, T.cnt, (size_t)kThCnt));
        if (n_anchors) VC_TRY(ensure(ctx, T.list, (size_t)n_anchors));
    }
    VC_TRY(pass_start(ctx, pass));
    uint32_t launches = 0, passes = 0, stable = 0;
    uint64_t removed_all = 0;
    // the launches of one stable compaction of n entries (compact) and of the words' record offsets (word_offsets)
    auto compact_launches = [](uint64_t n) { return 3u + ((n + kCompactGroup - 1) / kCompactGroup > kScanBlock ? 1u : 0u); };
    if (!S) { passes = 1; stable = 1; }                          // (one pass over nothing removes nothing)
    else {
        const dim3 block(kThBlock);
        const dim3 sgrid((uint32_t)((S + kThBlock - 1) / kThBlock));
        VC_HIP(ctx, hipMemcpyAsync(T.work.ptr, cur.words.ptr, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(T.anchor.ptr, 0, (size_t)nwords * sizeof(uint64_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(T.listed.ptr, 0, (size_t)nwords * sizeof(uint64_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(T.cnt.ptr, 0, kThCnt * sizeof(uint32_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(T.cnt.ptr + kThCntBad, 0xff, sizeof(uint32_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(T.peel.ptr, 0, (size_t)S * sizeof(uint16_t), ctx->stream));
        // item 5: the anchors' bits
        if (anchor_source != VC_THIN_ANCHORS_NONE) {
            if (n_anchors) {
                VC_HIP(ctx, hipMemcpyAsync(T.list.ptr, anchors, (size_t)n_anchors * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
                VC_DLAUNCH(kThinKind, k_thin_anchor, dim3((uint32_t)((n_anchors + kThBlock - 1) / kThBlock)), block, (const uint32_t *)T.list.ptr,
                           (uint32_t)n_anchors, n, (const unsigned long long *)cur.words.ptr, T.anchor.ptr, T.cnt.ptr);
                launches += 1;
            } else if (anchor_source == VC_THIN_ANCHORS_EXTREMA && ctx->geodesic.n == S) {
                VC_DLAUNCH(kThinKind, k_thin_pinned, sgrid, block, (const uint64_t *)cur.records.ptr, (const unsigned long long *)ctx->geodesic.key.ptr, S,
                           T.anchor.ptr);
                launches += 1;
            }
            VC_DLAUNCH(kThinKind, k_thin_count, dim3((uint32_t)((nwords + kThBlock - 1) / kThBlock)), block, (const unsigned long long *)T.anchor.ptr,
                       nwords, T.cnt.ptr);
            launches += 1;
            VC_HIP(ctx, hipGetLastError());
            VC_HIP(ctx, hipMemcpyAsync(T.h, T.cnt.ptr, kThCnt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (T.h[kThCntBad] != 0xffffffffu) {
                dist_harvest(ctx);
                const uint32_t bad = T.h[kThCntBad];
                return fail(ctx, VC_ERR_ARG, "vc_hull_thin: anchor %u (voxel %u) is no survivor", bad, bad < n_anchors ? anchors[bad] : 0u);
            }
            stats->anchors = T.h[kThCntAnchors];
        }
        if (T.use_table) VC_TRY(thin_table(ctx, &launches));
        ThParams p;
        memset(&p, 0, sizeof p);
        p.work = T.work.ptr; p.anchor = T.anchor.ptr; p.table = T.table.ptr; p.cnt = T.cnt.ptr; p.cand = T.cand.ptr; p.peel = T.peel.ptr;
        p.nwords = nwords; p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz; p.ncol = ctx->nx * ctx->ny;
        p.by_ncol = ms_divisor(p.ncol); p.by_ny = ms_divisor(p.ny);
        // the border list before the first pass; a voxel that joins it later takes its record from the words' record offsets
        VC_TRY(word_offsets(ctx, cur, nwords, T.woff, ctx->h_res + 1, kThinKind));
        launches += 3 + (word_groups(nwords) > kScanBlock ? 1 : 0);
        int at = 0;                                              // which of the two buffers holds the border list
        p.border = T.live[at].ptr; p.listed = T.listed.ptr; p.orig = reinterpret_cast<const unsigned long long *>(cur.words.ptr); p.woff = T.woff.ptr;
        VC_DLAUNCH(kThinKind, k_thin_border, sgrid, block, p, (const uint64_t *)cur.records.ptr, S);
        launches += 1;
        uint64_t blocks = (S + kThBlock - 1) / kThBlock;         // (the lists' counts stay on the device: the launches stride over them)
        if (blocks > kThMaxBlocks) blocks = kThMaxBlocks;
        const dim3 grid((uint32_t)blocks);
        while (passes < max_passes) {
            passes += 1;
            // item 4: six direction steps of a mark and eight sub-steps each
            VC_HIP(ctx, hipMemsetAsync(T.cnt.ptr, 0, (kThCntRemoved + 1) * sizeof(uint32_t), ctx->stream));
            for (uint32_t d = 0; d < 6; ++d) {
                const uint32_t code = 1u + 6u * (passes - 1u) + d;
                VC_DLAUNCH(kThinKind, k_thin_mark, grid, block, p, d);
                for (uint32_t s = 0; s < 8; ++s) {
                    if (T.use_table) VC_DLAUNCH(kThinKind, k_thin_sub<true>, grid, block, p, d, s, mode == VC_THIN_CURVE ? 1u : 0u, code);
                    else VC_DLAUNCH(kThinKind, k_thin_sub<false>, grid, block, p, d, s, mode == VC_THIN_CURVE ? 1u : 0u, code);
                }
                launches += 9;
            }
            VC_HIP(ctx, hipGetLastError());
            // the one read-back of the pass: how many it removed, and how long the border list has grown
            VC_HIP(ctx, hipMemcpyAsync(T.h + kThCntRemoved, T.cnt.ptr + kThCntRemoved, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const uint64_t removed = T.h[kThCntRemoved], listed = T.h[kThCntBorder];
            if (removed == 0) { stable = 1; break; }
            if (removed_all + removed >= S || removed > listed || listed > S) {
                dist_harvest(ctx);
                return fail(ctx, VC_ERR_INTERNAL, "vc_hull_thin: pass %u removed %llu of %llu listed voxels (%llu survivors, %llu removed before)", passes,
                            (unsigned long long)removed, (unsigned long long)listed, (unsigned long long)S, (unsigned long long)removed_all);
            }
            removed_all += removed;
            // the border list without them (vc_compact.h); its count goes back to the device
            ThSelLive sel;
            sel.live = T.live[at].ptr; sel.work = T.work.ptr; sel.out = T.live[at ^ 1].ptr;
            VC_TRY(compact(ctx, sel, listed, ctx->h_res));
            launches += compact_launches(listed);
            VC_HIP(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(T.cnt.ptr + kThCntBorder), (int)(uint32_t)(listed - removed), 1, ctx->stream));
            at ^= 1;
            p.border = T.live[at].ptr;
        }
        // item 6: the kept voxels in record order, their rows and the degree counts
        const uint64_t kept = S - removed_all;
        ThSelKept sel;
        sel.records = cur.records.ptr; sel.work = T.work.ptr; sel.out = T.live[at ^ 1].ptr;
        VC_TRY(compact(ctx, sel, S, ctx->h_res));
        launches += compact_launches(S);
        VC_DLAUNCH(kThinKind, k_thin_rows, dim3((uint32_t)((kept + kThBlock - 1) / kThBlock)), block, p, (const unsigned long long *)T.live[at ^ 1].ptr,
                   (uint32_t)kept, T.rows.ptr);
        launches += 1;
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(T.h, T.cnt.ptr, kThCnt * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    ctx->tm.thin_kernel_ms = 0;
    ctx->tm.thin_launches = 0;
    VC_TRY(pass_end(ctx, pass, &stats->thin_ms));
    ctx->tm.thin_ms = stats->thin_ms;
    const uint64_t live = S - removed_all;
    if (S && ctx->h_res[0] != live)
        return fail(ctx, VC_ERR_INTERNAL, "vc_hull_thin: %llu voxels kept of %llu, %llu removed", (unsigned long long)ctx->h_res[0], (unsigned long long)S,
                    (unsigned long long)removed_all);
    stats->survivors = S; stats->kept = live; stats->removed = removed_all;
    stats->passes = passes; stats->steps = T.h[kThCntSteps]; stats->launches = launches; stats->stable = stable;
    stats->isolated = T.h[kThCntIsolated]; stats->endpoints = T.h[kThCntEnds]; stats->junctions = T.h[kThCntJunctions];
    T.n = S; T.kept = live;
    T.stamp = ctx->result_gen;
    return VC_OK;
}

// The refusal the two fetch calls share.
static int thin_current(vc_ctx *ctx)
{
    if (!ctx->carved || !ctx->current(ctx->thin.stamp)) return fail(ctx, VC_ERR_ARG, "no skeleton: call vc_hull_thin on the current carve result");
    return VC_OK;
}

int vc_fetch_thin(vc_ctx *ctx, uint16_t *peel)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(thin_current(ctx));
    if (!peel || !ctx->thin.n) return VC_OK;     // (NULL: only asked whether the skeleton is valid)
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipMemcpy(peel, ctx->thin.peel.ptr, (size_t)ctx->thin.n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_skeleton(vc_ctx *ctx, vc_skeleton_voxel_t *out)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(thin_current(ctx));
    if (!out || !ctx->thin.kept) return VC_OK;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipMemcpy(out, ctx->thin.rows.ptr, (size_t)ctx->thin.kept * sizeof(vc_skeleton_voxel_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_thin_table(vc_ctx *ctx, uint8_t *bits)
{
    if (!ctx) return VC_ERR_ARG;
    if (!bits) return fail(ctx, VC_ERR_ARG, "vc_fetch_thin_table: bits must not be NULL");
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->dist_ev_kind.clear();
    VC_TRY(thin_table(ctx, nullptr));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->dist_ev_kind.clear();                   // (the table's launch belongs to no call's time)
    VC_HIP(ctx, hipMemcpy(bits, ctx->thin.table.ptr, VC_THIN_TABLE_BYTES, hipMemcpyDeviceToHost));
    return VC_OK;
}
