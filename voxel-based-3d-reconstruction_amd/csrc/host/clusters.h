// ---- the hull split into K figures on the floor plane (vc_clusters.h; contract in include/voxcarve.h) ----
// d_cl_acc: [0, 4) Wtot, sum w Px, sum w Py, columns; [4, 20) the seeds' largest keys; [20, 36) voxels per cluster; [36, 100) the
// round's {W_k, sum w Px, sum w Py, columns}.  d_cl_box: lo [K][3], then hi [K][3].
constexpr uint32_t kClAccSeed = 4, kClAccVoxels = 20, kClAccRound = 36, kClAccTotal = kClAccRound + kClMaxK * kClAcc;
constexpr uint32_t kClHostBox = kClMaxK * 6 / 2;               // the boxes read back behind the accumulators, as u64

int vc_hull_clusters(vc_ctx *ctx, uint32_t K, uint32_t max_iters, uint32_t min_column, uint32_t hist_iz_lo, uint32_t hist_iz_hi,
                     const int64_t *init, uint32_t flags, vc_cluster_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: flags must be 0 (got %u)", flags);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_clusters", "label", "clustering", pass));
    if (K < 1 || K > kClMaxK) return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: K = %u not in [1, %u]", K, kClMaxK);
    if (max_iters < 1 || max_iters > 255) return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: max_iters %u not in [1, 255]", max_iters);
    if (hist_iz_lo > hist_iz_hi || hist_iz_hi >= ctx->nz)
        return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: the band [%u, %u] of the colour signature is not inside the grid's %u layers",
                    hist_iz_lo, hist_iz_hi, ctx->nz);
    if (init)
        for (uint32_t k = 0; k < 2 * K; ++k)
            if (init[k] > (1ll << 30) || init[k] < -(1ll << 30))
                return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: init centre %u has %c = %lld um, beyond +-2^30", k / 2, "xy"[k & 1], (long long)init[k]);
    uint64_t q[2];
    VC_TRY(dist_metric(ctx, "vc_hull_clusters", q, 2));
    const uint64_t S = pass.S, n = pass.n, ncol64 = (uint64_t)ctx->nx * ctx->ny;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_clusters: %llu voxels exceed the u32 index", (unsigned long long)n);
    const uint32_t ncol = (uint32_t)ncol64;
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->clusters.stamp = kNever;
    VC_HIP(ctx, ensure_pinned(ctx->clusters.h, kClAccTotal + kClHostBox));
    VC_TRY(ensure(ctx, ctx->clusters.fmap, (size_t)ncol));
    VC_TRY(ensure(ctx, ctx->clusters.flab, (size_t)ncol));
    VC_TRY(ensure(ctx, ctx->clusters.lab, (size_t)S));
    VC_TRY(ensure(ctx, ctx->clusters.hist, (size_t)kClMaxK * kClBins));
    VC_TRY(ensure(ctx, ctx->clusters.box, (size_t)kClMaxK * 6));
    VC_TRY(ensure(ctx, ctx->clusters.seed, (size_t)kClMaxK));
    VC_TRY(ensure(ctx, ctx->clusters.acc, (size_t)kClAccTotal));
    uint32_t *blo = ctx->clusters.box.ptr, *bhi = blo + kClMaxK * 3;
    uint64_t *h = ctx->clusters.h;
    VC_TRY(pass_start(ctx, pass, kWordsLater));     // (only the floor map made from the occupancy reads the words)
    VC_HIP(ctx, hipMemsetAsync(ctx->clusters.fmap.ptr, 0, (size_t)ncol * sizeof(uint32_t), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(ctx->clusters.flab.ptr, 0xff, (size_t)ncol, ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(ctx->clusters.hist.ptr, 0, (size_t)kClMaxK * kClBins * sizeof(uint32_t), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(blo, 0xff, (size_t)kClMaxK * 3 * sizeof(uint32_t), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(bhi, 0, (size_t)kClMaxK * 3 * sizeof(uint32_t), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(ctx->clusters.seed.ptr, 0xff, (size_t)kClMaxK * sizeof(uint32_t), ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(ctx->clusters.acc.ptr, 0, (size_t)kClAccTotal * sizeof(uint64_t), ctx->stream));
    ClCols cols;
    memset(&cols, 0, sizeof cols);
    cols.fmap = ctx->clusters.fmap.ptr; cols.ncol = ncol; cols.ny = ctx->ny; cols.min_column = min_column;
    cols.qx = (long long)q[0]; cols.qy = (long long)q[1];
    const dim3 block(kClBlock);
    const uint64_t cblocks = (ncol64 + kClBlock - 1) / kClBlock;
    const dim3 cgrid((uint32_t)(cblocks < kClMaxBlocks ? cblocks : kClMaxBlocks));
    unsigned long long *acc = ctx->clusters.acc.ptr;
    memset(h, 0, (kClAccTotal + kClHostBox) * sizeof(uint64_t));
    if (S) {
        // item 2: the floor map and its moments
        if (ctx->clusters.floor_records) {
            hipLaunchKernelGGL(k_cl_floor_records, dim3((uint32_t)((S + kClBlock - 1) / kClBlock)), block, 0, ctx->stream,
                               (const uint64_t *)cur.records.ptr, S, ncol, ctx->clusters.fmap.ptr);
        } else {
            VC_TRY(densify_words(ctx, cur));
            const uint32_t ngroups = (uint32_t)((ncol64 + 63) / 64), nchunks = (ctx->nz + kClLayers - 1) / kClLayers;
            const uint64_t waves = (uint64_t)ngroups * nchunks;
            hipLaunchKernelGGL(k_cl_floor, dim3((uint32_t)((waves + kClBlock / 64 - 1) / (kClBlock / 64))), block, 0, ctx->stream,
                               (const uint64_t *)cur.words.ptr, pass.nwords, ncol, ctx->nz, ngroups, nchunks, ctx->clusters.fmap.ptr);
        }
        VC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_cl_moments, cgrid, block, 0, ctx->stream, cols, acc);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(h, acc, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    const uint64_t Wtot = h[0], columns = h[3];
    if (Wtot > S || columns > S || h[1] >= (1ull << 62) || h[2] >= (1ull << 62))
        return fail(ctx, VC_ERR_HIP, "vc_hull_clusters: the floor map weighs %llu in %llu columns, the result has %llu records",
                    (unsigned long long)Wtot, (unsigned long long)columns, (unsigned long long)S);
    ClCentres c;
    memset(&c, 0, sizeof c);
    if (init) for (uint32_t k = 0; k < K; ++k) { c.c[k][0] = init[2 * k]; c.c[k][1] = init[2 * k + 1]; }
    if (Wtot && !init) {
        // item 3: two launches per seed, the seeds' columns stay on the device until all are picked
        ClSeed sd;
        memset(&sd, 0, sizeof sd);
        sd.seedcol = ctx->clusters.seed.ptr; sd.pick = ctx->clusters.seed.ptr; sd.best = acc + kClAccSeed;
        sd.mx = (long long)((h[1] + Wtot / 2) / Wtot); sd.my = (long long)((h[2] + Wtot / 2) / Wtot);
        for (uint32_t j = 0; j < K; ++j) {
            sd.j = j;
            hipLaunchKernelGGL(k_cl_seed_best, cgrid, block, 0, ctx->stream, cols, sd);
            hipLaunchKernelGGL(k_cl_seed_pick, cgrid, block, 0, ctx->stream, cols, sd);
            VC_HIP(ctx, hipGetLastError());
        }
        VC_HIP(ctx, hipMemcpyAsync(h + 4, ctx->clusters.seed.ptr, kClMaxK * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t *sc = reinterpret_cast<const uint32_t *>(h + 4);
        for (uint32_t k = 0; k < K; ++k) {
            if (sc[k] >= ncol) return fail(ctx, VC_ERR_HIP, "vc_hull_clusters: seed %u fell on column %u of %u", k, sc[k], ncol);
            c.c[k][0] = (long long)q[0] * (sc[k] / ctx->ny); c.c[k][1] = (long long)q[1] * (sc[k] % ctx->ny);
        }
    }
    // item 4: one launch and 8 K words back per round
    uint32_t r = 0;
    bool converged = Wtot == 0;
    uint64_t *hr = h + kClAccRound;
    memset(hr, 0, kClMaxK * kClAcc * sizeof(uint64_t));
    while (Wtot && r < max_iters) {
        ++r;
        VC_HIP(ctx, hipMemsetAsync(acc + kClAccRound, 0, kClMaxK * kClAcc * sizeof(uint64_t), ctx->stream));
        hipLaunchKernelGGL(k_cl_round, cgrid, block, 0, ctx->stream, cols, K, c, ctx->clusters.flab.ptr, acc + kClAccRound);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(hr, acc + kClAccRound, kClMaxK * kClAcc * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        bool changed = false;
        for (uint32_t k = 0; k < K; ++k) {
            const uint64_t W = hr[kClAcc * k];
            if (!W) continue;
            if (W > Wtot) return fail(ctx, VC_ERR_HIP, "vc_hull_clusters: cluster %u weighs %llu of %llu", k, (unsigned long long)W, (unsigned long long)Wtot);
            const long long x = (long long)((hr[kClAcc * k + 1] + W / 2) / W), y = (long long)((hr[kClAcc * k + 2] + W / 2) / W);
            changed |= x != c.c[k][0] || y != c.c[k][1];
            c.c[k][0] = x; c.c[k][1] = y;
        }
        if (!changed) { converged = true; break; }
    }
    if (S && !Wtot) {
        // no column reaches min_column: no rounds, every record takes label 0 (one cluster's launch; its weights are zero)
        VC_HIP(ctx, hipMemsetAsync(acc + kClAccRound, 0, kClMaxK * kClAcc * sizeof(uint64_t), ctx->stream));
        hipLaunchKernelGGL(k_cl_round, cgrid, block, 0, ctx->stream, cols, 1u, c, ctx->clusters.flab.ptr, acc + kClAccRound);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(hr, acc + kClAccRound, kClMaxK * kClAcc * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (S) {
        // item 5: voxels and boxes from the columns, labels, histograms and iz ranges from the records
        hipLaunchKernelGGL(k_cl_columns, cgrid, block, 0, ctx->stream, cols, K, (const uint8_t *)ctx->clusters.flab.ptr, acc + kClAccVoxels, blo, bhi);
        VC_HIP(ctx, hipGetLastError());
        ClRecords p;
        memset(&p, 0, sizeof p);
        p.records = cur.records.ptr; p.flab = ctx->clusters.flab.ptr; p.lab = ctx->clusters.lab.ptr; p.hist = ctx->clusters.hist.ptr;
        p.blo = blo; p.bhi = bhi;
        p.S = S; p.ncol = ncol; p.K = K; p.zlo = hist_iz_lo; p.zhi = hist_iz_hi;
        const uint64_t rblocks = (S + kClBlock - 1) / kClBlock, rgrid = rblocks < kClMaxBlocks ? rblocks : kClMaxBlocks;
        p.per = ((S + rgrid - 1) / rgrid + kClBlock - 1) / kClBlock * kClBlock;
        hipLaunchKernelGGL(k_cl_records, dim3((uint32_t)rgrid), block, 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(h + kClAccVoxels, acc + kClAccVoxels, kClMaxK * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipMemcpyAsync(h + kClAccTotal, blo, kClMaxK * 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    VC_TRY(pass_end(ctx, pass, &stats->clusters_ms));
    const uint32_t *hb = reinterpret_cast<const uint32_t *>(h + kClAccTotal);     // lo [kClMaxK][3], hi [kClMaxK][3] (zeros when S = 0)
    ctx->clusters.out.assign(K, vc_cluster_t{});
    uint64_t labelled = 0;
    for (uint32_t k = 0; k < K; ++k) {
        vc_cluster_t &o = ctx->clusters.out[k];
        o.centre_um[0] = c.c[k][0]; o.centre_um[1] = c.c[k][1];
        o.voxels = S ? h[kClAccVoxels + k] : 0;
        o.weight = hr[kClAcc * k];
        o.columns = (uint32_t)hr[kClAcc * k + 3];
        for (int a = 0; a < 3; ++a) {
            o.lo[a] = o.voxels ? hb[3 * k + a] : 0xffffffffu;
            o.hi[a] = o.voxels ? hb[kClMaxK * 3 + 3 * k + a] : 0u;
        }
        labelled += o.voxels;
    }
    if (labelled != S)
        return fail(ctx, VC_ERR_HIP, "vc_hull_clusters: the occupancy holds %llu voxels, the result %llu records", (unsigned long long)labelled,
                    (unsigned long long)S);
    stats->survivors = S;
    stats->columns = columns;
    stats->weight = Wtot;
    stats->iterations = r;
    stats->converged = converged ? 1u : 0u;
    stats->q[0] = q[0]; stats->q[1] = q[1];
    ctx->clusters.stamp = ctx->result_gen;
    ctx->clusters.n = S; ctx->clusters.k = K; ctx->clusters.ncol = ncol;
    return VC_OK;
}

// The refusal the fetch calls and vc_paint_clusters share.
static int clusters_current(vc_ctx *ctx)
{
    if (!ctx->carved || !ctx->current(ctx->clusters.stamp)) return fail(ctx, VC_ERR_ARG, "no clusters: call vc_hull_clusters on the current carve result");
    return VC_OK;
}

int vc_fetch_cluster_labels(vc_ctx *ctx, uint8_t *labels)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(clusters_current(ctx));
    if (!labels) return VC_OK;                   // only asked whether the clustering is valid
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->clusters.n) VC_HIP(ctx, hipMemcpy(labels, ctx->clusters.lab.ptr, (size_t)ctx->clusters.n, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_clusters(vc_ctx *ctx, vc_cluster_t *out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    VC_TRY(clusters_current(ctx));
    memcpy(out, ctx->clusters.out.data(), ctx->clusters.out.size() * sizeof(vc_cluster_t));
    return VC_OK;
}

int vc_fetch_cluster_histograms(vc_ctx *ctx, uint32_t *hist)
{
    if (!ctx || !hist) return VC_ERR_ARG;
    VC_TRY(clusters_current(ctx));
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipMemcpy(hist, ctx->clusters.hist.ptr, (size_t)ctx->clusters.k * kClBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_floor_map(vc_ctx *ctx, uint32_t *n)
{
    if (!ctx || !n) return VC_ERR_ARG;
    VC_TRY(clusters_current(ctx));
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipMemcpy(n, ctx->clusters.fmap.ptr, (size_t)ctx->clusters.ncol * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_floor_labels(vc_ctx *ctx, uint8_t *labels)
{
    if (!ctx || !labels) return VC_ERR_ARG;
    VC_TRY(clusters_current(ctx));
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_HIP(ctx, hipMemcpy(labels, ctx->clusters.flab.ptr, (size_t)ctx->clusters.ncol, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_paint_clusters(vc_ctx *ctx, const uint8_t *rgb)
{
    if (!ctx) return VC_ERR_ARG;
    if (!rgb) return fail(ctx, VC_ERR_ARG, "vc_paint_clusters: no palette");
    VC_TRY(clusters_current(ctx));
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->clusters.n) return VC_OK;
    StepBuf &cur = ctx->sb[ctx->cur];
    VC_HIP(ctx, hipSetDevice(ctx->device));
    ClPalette pal;
    memset(&pal, 0, sizeof pal);
    for (uint32_t k = 0; k < ctx->clusters.k; ++k) pal.rgb[k] = (uint32_t)rgb[3 * k] | ((uint32_t)rgb[3 * k + 1] << 8) | ((uint32_t)rgb[3 * k + 2] << 16);
    hipLaunchKernelGGL(k_cl_paint, dim3((uint32_t)((ctx->clusters.n + kClBlock - 1) / kClBlock)), dim3(kClBlock), 0, ctx->stream, cur.records.ptr,
                       ctx->clusters.n, (const uint8_t *)ctx->clusters.lab.ptr, pal);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VC_OK;
}
