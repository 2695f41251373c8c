// ---- the vote over the last frames' hulls, aligned by block motion first (vc_temporal_motion.h; contract in include/voxcarve.h) ----
// Ring, P, staging buffer, counters and the record hand-over are vc_hull_temporal's; the field is motion.h's motion_field between the
// result's words and the ring's newest snapshot, kept in a state of the vote's own.
int vc_hull_temporal_motion(vc_ctx *ctx, uint32_t window, uint32_t keep_on, uint32_t keep_off, uint32_t block, uint32_t apron, uint32_t search,
                            uint32_t flags, vc_temporal_motion_stats_t *stats)
{
    static const char *const what = "vc_hull_temporal_motion";
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "%s: stats must not be NULL", what);
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "%s: flags must be 0 (got %u)", what, flags);
    Pass pass;
    VC_TRY(pass_open(ctx, what, "vote on", "temporal voting", pass));
    if (window < 1 || window > VC_TEMPORAL_MAX_WINDOW) return fail(ctx, VC_ERR_ARG, "%s: window %u not in [1, %u]", what, window, VC_TEMPORAL_MAX_WINDOW);
    if (keep_on < 1 || keep_on > window) return fail(ctx, VC_ERR_ARG, "%s: keep_on %u not in [1, window = %u]", what, keep_on, window);
    if (keep_off < 1 || keep_off > keep_on) return fail(ctx, VC_ERR_ARG, "%s: keep_off %u not in [1, keep_on = %u]", what, keep_off, keep_on);
    StepBuf &cur = *pass.cur;
    const uint64_t n = pass.n, nwords = pass.nwords, npad = (nwords + 1) & ~1ull;
    MotionGrid g;
    VC_TRY(motion_grid(ctx, what, block, apron, search, n, nwords, g));
    VC_TRY(merge_refuse_slot(ctx, what, cur));
    vc_ctx::Temporal &T = ctx->temporal;
    if (ctx->current(T.stamp))
        return fail(ctx, VC_ERR_ARG, "%s: the current result is already the last call's output (one push per result): carve again first", what);
    if (cur.words.cap < npad) return fail(ctx, VC_ERR_INTERNAL, "%s: the result's %llu occupancy words are not padded to %llu", what,
                                          (unsigned long long)cur.words.cap, (unsigned long long)npad);
    VC_TRY(pass_begin(ctx));
    // a ring of another window, another grid or the other kind of call starts over; its buffers are made beside the old ones, which
    // stay until the call commits
    const bool restart = T.pushes == 0 || T.window != window || T.nwords != nwords || !T.aligned;
    const size_t rwords = (size_t)window * npad;
    const bool alloc = T.ring.cap < rwords || T.ring2.cap < rwords || T.prev.cap < npad || T.stage.cap < npad || !T.ring.ptr || !T.ring2.ptr;
    DevBuf<uint64_t> ring_n, ring2_n, prev_n, stage_n;
    if (alloc) {
        if (!restart) return fail(ctx, VC_ERR_INTERNAL, "%s: the rings hold %zu and %zu words, %u x %llu are in use", what, T.ring.cap, T.ring2.cap, window,
                                  (unsigned long long)npad);
        VC_TRY(ensure(ctx, ring_n, rwords));
        VC_TRY(ensure(ctx, ring2_n, rwords));
        VC_TRY(ensure(ctx, prev_n, (size_t)npad));
        VC_TRY(ensure(ctx, stage_n, (size_t)npad));
    }
    VC_TRY(ensure(ctx, T.ctr, 8));
    VC_HIP(ctx, ensure_pinned(T.h, 8));
    vc_ctx::Motion &F = T.field;
    VC_TRY(motion_sized(ctx, F, g));
    const uint64_t have = restart ? 0 : std::min<uint64_t>(T.pushes, window);     // snapshots in the ring
    const uint32_t m = (uint32_t)std::min<uint64_t>(have + 1, window);
    const uint32_t on = (keep_on * m + window - 1) / window, off = (keep_off * m + window - 1) / window;
    const uint64_t S0 = pass.S;
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    // the field from the ring's newest snapshot (the raw H_{t-1}) to H_t; the first read-back, the listed blocks, is in there
    uint64_t listed = 0;
    if (have) VC_TRY(motion_field(ctx, what, F, g, cur.words.ptr, T.ring.ptr + (size_t)T.head * npad, listed));
    else VC_HIP(ctx, hipMemsetAsync(F.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    TemporalAlignParams ap;
    memset(&ap, 0, sizeof ap);
    ap.ring = have ? T.ring.ptr : nullptr;
    ap.ring2 = have ? T.ring2.ptr : nullptr;
    ap.cur = cur.words.ptr;
    ap.prev = have ? T.prev.ptr : nullptr;
    ap.vec = have ? F.vec.ptr : nullptr;
    ap.stage = alloc ? stage_n.ptr : T.stage.ptr;
    ap.ctr = T.ctr.ptr;
    ap.g = g; ap.npad = npad;
    ap.window = window; ap.head = have ? T.head : 0;
    ap.count = m - 1;                            // min(have, window - 1): the ring's oldest slot is read only while the ring fills
    ap.on = on; ap.off = off;
    VC_HIP(ctx, hipMemsetAsync(T.ctr.ptr, 0, 8 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_temporal_align_vote, dim3((uint32_t)((npad + kSetopBlock - 1) / kSetopBlock)), dim3(kSetopBlock), 0, ctx->stream, ap);
    VC_HIP(ctx, hipGetLastError());
    // the second read-back: |O_t| sizes the records; the field's counters come with it
    VC_HIP(ctx, hipMemcpyAsync(T.h.ptr, T.ctr.ptr, kAlignCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipMemcpyAsync(F.h.ptr, F.ctr.ptr, kMotionCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t S1 = T.h[0], added = T.h[1], removed = T.h[2], raw_changed = T.h[3], out_changed = T.h[4], aligned_changed = T.h[5];
    if (S1 > n || removed > S0 || S0 + added - removed != S1)
        return fail(ctx, VC_ERR_HIP, "%s: %llu voted in, %llu added to and %llu removed from %llu survivors, in a grid of %llu voxels", what,
                    (unsigned long long)S1, (unsigned long long)added, (unsigned long long)removed, (unsigned long long)S0, (unsigned long long)n);
    if (motion_counters_bad(F, listed))
        return fail(ctx, VC_ERR_HIP, "%s: %llu moved, %llu unique, %llu clipped of %llu listed blocks, cost %llu -> %llu", what, (unsigned long long)F.h[0],
                    (unsigned long long)F.h[1], (unsigned long long)F.h[2], (unsigned long long)listed, (unsigned long long)F.h[3], (unsigned long long)F.h[4]);
    const bool changed = added || removed;
    // every buffer of the hand-over before anything is committed: a failure leaves result, ring and P
    VC_TRY(ensure(ctx, T.votes, (size_t)S1));
    VC_TRY(ensure(ctx, T.added, (size_t)S1));
    MergeParams mg;
    VC_TRY(merge_sized(ctx, cur, nwords, S1, changed, T.added.ptr, mg));
    // committed from here on: the aligned ring becomes the ring and takes H_t, the result O_t, P the staging buffer
    T.stamp = kNever;
    if (alloc) { T.ring = std::move(ring_n); T.ring2 = std::move(ring2_n); T.prev = std::move(prev_n); T.stage = std::move(stage_n); }
    if (restart) {
        VC_HIP(ctx, hipMemsetAsync(T.ring.ptr, 0, rwords * sizeof(uint64_t), ctx->stream));    // (the slots' pads stay zero, in both rings)
        VC_HIP(ctx, hipMemsetAsync(T.ring2.ptr, 0, rwords * sizeof(uint64_t), ctx->stream));
        T.window = window; T.nwords = nwords; T.npad = npad;
        T.head = window - 1;
        T.pushes = 0;
        T.aligned = true;
    } else {
        std::swap(T.ring, T.ring2);              // (the launch above holds the pointers it was given)
    }
    T.head = (T.head + 1) % window;
    T.pushes += 1;
    VC_HIP(ctx, hipMemcpyAsync(T.ring.ptr + (size_t)T.head * npad, cur.words.ptr, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(T.added.ptr, 0, std::max<size_t>((size_t)S1, 1), ctx->stream));
    TemporalParams tp;
    memset(&tp, 0, sizeof tp);
    tp.ring = T.ring.ptr; tp.stage = ap.stage; tp.ctr = T.ctr.ptr;
    tp.nwords = nwords; tp.npad = npad; tp.n = n;
    tp.window = window; tp.head = T.head; tp.count = m; tp.on = on; tp.off = off;
    const dim3 gblock(kMergeBlock), wgrid((uint32_t)((nwords + kMergeBlock - 1) / kMergeBlock));
    if (changed) {
        result_changed(ctx);
        VC_HIP(ctx, hipMemcpyAsync(cur.words.ptr, tp.stage, (size_t)nwords * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (changed || S1) VC_TRY(merge_ranked(ctx, cur, mg, nwords, S0, changed, VC_K_TEMPORAL_RANK, VC_K_TEMPORAL_MERGE));
    if (changed && S1) VC_DLAUNCH(VC_K_TEMPORAL_MERGE, k_temporal_new<true>, wgrid, gblock, mg, tp, T.votes.ptr);
    else if (S1) VC_DLAUNCH(VC_K_TEMPORAL_RANK, k_temporal_new<false>, wgrid, gblock, mg, tp, T.votes.ptr);
    VC_HIP(ctx, hipGetLastError());
    if (changed) VC_TRY(records_handed_over(ctx, cur, word_groups(nwords)));
    std::swap(T.prev, T.stage);                  // (the launches above hold the pointers they were given)
    VC_TRY(pass_end(ctx, pass, &stats->temporal_ms));
    if (changed) ctx->survivors = cur.survivors = S1;
    if (changed || S1) VC_TRY(merge_counted(ctx, what, S1, "were voted in"));
    stats->window = window; stats->frames = m; stats->on = on; stats->off = off;
    stats->block = block; stats->apron = apron; stats->search = search;
    stats->survivors_before = S0; stats->survivors_after = S1;
    stats->added = added; stats->removed = removed;
    stats->raw_changed = raw_changed; stats->aligned_changed = aligned_changed; stats->out_changed = out_changed;
    stats->blocks = g.nblocks; stats->listed = listed;
    if (have) {
        stats->moved = F.h[0]; stats->unique = F.h[1]; stats->clipped = F.h[2]; stats->cost0_sum = F.h[3]; stats->cost_sum = F.h[4];
    }
    F.g = g; F.listed = listed;
    T.has_field = true;
    T.stamp = ctx->result_gen;
    T.n = S1;
    return VC_OK;
}

int vc_fetch_temporal_motion(vc_ctx *ctx, vc_motion_t *rows, uint64_t *count)
{
    if (!ctx) return VC_ERR_ARG;
    const vc_ctx::Temporal &T = ctx->temporal;
    if (!ctx->carved || !ctx->current(T.stamp) || !T.has_field)
        return fail(ctx, VC_ERR_ARG, "no field: call vc_hull_temporal_motion on the current carve result");
    if (count) *count = T.field.listed;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (rows && T.field.listed)
        VC_HIP(ctx, hipMemcpy(rows, T.field.rows.ptr, (size_t)T.field.listed * sizeof(vc_motion_t), hipMemcpyDeviceToHost));
    return VC_OK;
}
