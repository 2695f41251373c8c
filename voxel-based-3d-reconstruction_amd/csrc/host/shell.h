// ---- the hull's shell: the cells with an exposed face, their faces, levels of detail (vc_shell.h; contract in include/voxcarve.h) ----
static ShGrid shell_grid(const uint32_t *words32, uint64_t nw32, uint32_t nx, uint32_t ny, uint32_t nz)
{
    ShGrid g;
    memset(&g, 0, sizeof g);
    g.words32 = words32; g.nw32 = nw32;
    g.nx = nx; g.ny = ny; g.nz = nz; g.ncol = nx * ny;
    g.by_ncol = ms_divisor(g.ncol); g.by_ny = ms_divisor(ny);
    return g;
}

int vc_hull_shell(vc_ctx *ctx, uint32_t level, uint32_t flags, vc_shell_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_shell: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_shell: flags must be 0 (got %u)", flags);
    if (level > VC_SHELL_MAX_LEVEL) return fail(ctx, VC_ERR_ARG, "vc_hull_shell: level %u not in 0..%u", level, VC_SHELL_MAX_LEVEL);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_shell", "list the shell of", "shell listing", pass));
    const uint64_t S = pass.S, n = pass.n, nwords = pass.nwords;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_shell: %llu voxels exceed the u32 index", (unsigned long long)n);
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    vc_ctx::Shell &sh = ctx->shell;
    sh.stamp = kNever;
    const uint32_t L = level, f = 1u << L;
    const uint32_t cnx = (ctx->nx + f - 1) / f, cny = (ctx->ny + f - 1) / f, cnz = (ctx->nz + f - 1) / f;
    const uint64_t cn = (uint64_t)cnx * cny * cnz, nwc = (cn + 63) / 64;
    const uint32_t rgroups = (uint32_t)((S + kCompactGroup - 1) / kCompactGroup), cgroups = word_groups(nwc);
    VC_HIP(ctx, ensure_pinned(sh.h, kShCounters));
    VC_TRY(ensure(ctx, sh.cnt, kShCounters));
    if (S) {
        VC_TRY(ensure(ctx, ctx->d_rscan, rgroups > cgroups ? rgroups : cgroups));
        VC_TRY(ensure(ctx, sh.fb, (size_t)S));
        if (L) {
            VC_TRY(ensure(ctx, sh.cwords, (size_t)nwc));
            VC_TRY(ensure(ctx, sh.shw, (size_t)nwc));
            VC_TRY(ensure(ctx, sh.woff, (size_t)nwc));
        }
    }
    VC_TRY(pass_start(ctx, pass));
    VC_HIP(ctx, hipMemsetAsync(sh.cnt.ptr, 0, kShCounters * sizeof(uint64_t), ctx->stream));
    uint64_t T = 0;
    if (S) {
        const dim3 block(kShBlock), sgrid((uint32_t)((S + kShBlock - 1) / kShBlock)), wgrid((uint32_t)((nwc + kShBlock - 1) / kShBlock));
        const dim3 cgrid((cgroups + kCcBlock / 64 - 1) / (kCcBlock / 64));
        const ShGrid fine = shell_grid(reinterpret_cast<const uint32_t *>(cur.words.ptr), 2 * nwords, ctx->nx, ctx->ny, ctx->nz);
        const ShGrid coarse = shell_grid(reinterpret_cast<const uint32_t *>(sh.cwords.ptr), 2 * nwc, cnx, cny, cnz);
        const ShLevel lev = {L, cnx, cny};
        // the level-0 face bytes: at level 0 with the counts of the compaction, above it with the coarse cells' bits
        if (!L) {
            const ShSel0<true> first = {fine, cur.records.ptr, sh.fb.ptr, nullptr, nullptr, 0};
            hipLaunchKernelGGL(k_compact_count<ShSel0<true>>, dim3(rgroups), dim3(kCompactBlock), 0, ctx->stream, S, ctx->d_rscan.cnt.ptr, first);
            VC_HIP(ctx, hipGetLastError());
        } else {
            VC_HIP(ctx, hipMemsetAsync(sh.cwords.ptr, 0, (size_t)nwc * sizeof(uint64_t), ctx->stream));
            hipLaunchKernelGGL(k_sh_mark, sgrid, block, 0, ctx->stream, (const uint64_t *)cur.records.ptr, S, fine, lev, sh.fb.ptr,
                               reinterpret_cast<uint32_t *>(sh.cwords.ptr), 2 * nwc);
            hipLaunchKernelGGL(k_sh_cshell, wgrid, block, 0, ctx->stream, coarse, (const uint64_t *)sh.cwords.ptr, nwc, sh.shw.ptr,
                               sh.cnt.ptr + 6);
            hipLaunchKernelGGL(k_cc_wcount, cgrid, dim3(kCcBlock), 0, ctx->stream, (const uint64_t *)sh.shw.ptr, nwc, cgroups, ctx->d_rscan.cnt.ptr);
            VC_HIP(ctx, hipGetLastError());
        }
        VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_rscan, ctx->d_rscan.cnt.ptr, L ? cgroups : rgroups, ctx->h_res + 0));
        // the one read-back before the end: the number of shell cells sizes their buffers
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        T = ctx->h_res[0];
        if (T > S || T > cn) return fail(ctx, VC_ERR_HIP, "vc_hull_shell: %llu shell cells of %llu survivors", (unsigned long long)T, (unsigned long long)S);
        if (T) {
            VC_TRY(ensure(ctx, sh.rec, (size_t)T));
            VC_TRY(ensure(ctx, sh.faces, (size_t)T));
            if (L) VC_TRY(ensure(ctx, sh.acc, (size_t)T * 4));
        }
        const uint32_t *off = ctx->d_rscan.off.ptr;
        const uint64_t *boff = ctx->d_rscan.boff.ptr;
        if (T && !L) {
            const ShSel0<false> second = {fine, cur.records.ptr, sh.fb.ptr, sh.rec.ptr, sh.faces.ptr, T};
            hipLaunchKernelGGL(k_compact_scatter<ShSel0<false>>, dim3(rgroups), dim3(kCompactBlock), 0, ctx->stream, S, off, boff, second);
        } else if (T) {
            const dim3 tgrid((uint32_t)((T + kShBlock - 1) / kShBlock));
            hipLaunchKernelGGL(k_cc_woff, cgrid, dim3(kCcBlock), 0, ctx->stream, (const uint64_t *)sh.shw.ptr, nwc, cgroups, off, boff, sh.woff.ptr);
            VC_HIP(ctx, hipMemsetAsync(sh.acc.ptr, 0, (size_t)T * 4 * sizeof(uint32_t), ctx->stream));
            hipLaunchKernelGGL(k_sh_emit, wgrid, block, 0, ctx->stream, coarse, (const uint64_t *)sh.shw.ptr, nwc, (const uint32_t *)sh.woff.ptr,
                               sh.rec.ptr, sh.faces.ptr, T);
            hipLaunchKernelGGL(k_sh_accum, sgrid, block, 0, ctx->stream, (const uint64_t *)cur.records.ptr, (const uint8_t *)sh.fb.ptr, S, fine, lev,
                               (const uint64_t *)sh.shw.ptr, nwc, (const uint32_t *)sh.woff.ptr, sh.acc.ptr, T);
            hipLaunchKernelGGL(k_sh_final, tgrid, block, 0, ctx->stream, (const uint32_t *)sh.acc.ptr, sh.rec.ptr, T);
        }
        if (T) {
            const uint64_t blocks = (T + kShBlock - 1) / kShBlock;
            hipLaunchKernelGGL(k_sh_fcount, dim3((uint32_t)(blocks < kShCountBlocks ? blocks : kShCountBlocks)), block, 0, ctx->stream,
                               (const uint8_t *)sh.faces.ptr, T, sh.cnt.ptr);
        }
        VC_HIP(ctx, hipGetLastError());
    }
    VC_HIP(ctx, hipMemcpyAsync(sh.h, sh.cnt.ptr, kShCounters * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->shell_ms));
    stats->survivors = S; stats->cells_on = L ? sh.h[6] : S; stats->shell = T;
    for (int k = 0; k < 6; ++k) stats->faces[k] = sh.h[k];
    stats->level = L; stats->cube_scale = f;
    stats->dims[0] = cnx; stats->dims[1] = cny; stats->dims[2] = cnz;
    sh.T = T; sh.level = L;
    sh.dims[0] = cnx; sh.dims[1] = cny; sh.dims[2] = cnz;
    sh.stamp = ctx->result_gen;
    return VC_OK;
}

// The refusal the two fetch calls share.
static int shell_current(vc_ctx *ctx)
{
    if (!ctx->carved || !ctx->current(ctx->shell.stamp)) return fail(ctx, VC_ERR_ARG, "no shell: call vc_hull_shell on the current carve result");
    return VC_OK;
}

int vc_fetch_shell(vc_ctx *ctx, uint64_t *records, uint8_t *faces)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(shell_current(ctx));
    const vc_ctx::Shell &sh = ctx->shell;
    if (!sh.T || (!records && !faces)) return VC_OK;            // (both NULL: only asked whether the shell is valid)
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (records) VC_HIP(ctx, hipMemcpy(records, sh.rec.ptr, (size_t)sh.T * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (faces) VC_HIP(ctx, hipMemcpy(faces, sh.faces.ptr, (size_t)sh.T, hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_shell_viewer(vc_ctx *ctx, double scaling, float *positions, float *colors)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(shell_current(ctx));
    if (!std::isfinite(scaling) || scaling == 0.0) return fail(ctx, VC_ERR_ARG, "vc_fetch_shell_viewer: scaling %g is zero or not finite", scaling);
    vc_ctx::Shell &sh = ctx->shell;
    if (!sh.T || (!positions && !colors)) return VC_OK;
    VC_HIP(ctx, hipSetDevice(ctx->device));
    // item 4 of the contract in float64 on the host: per axis and (coarse) cell the midpoint of its first and last voxel's
    // truncated, scaled coordinate (z negated: the viewer's y points up), per colour byte c / 255
    const uint32_t f = 1u << sh.level, fine[3] = {ctx->nx, ctx->ny, ctx->nz};
    const std::vector<double> *axes[3] = {&ctx->xs, &ctx->ys, &ctx->zs};
    std::vector<float> tab;
    tab.reserve((size_t)sh.dims[0] + sh.dims[1] + sh.dims[2] + 256);
    for (int a = 0; a < 3; ++a)
        for (uint32_t c = 0; c < sh.dims[a]; ++c) {
            const uint64_t lo = (uint64_t)f * c, end = lo + f < fine[a] ? lo + f : fine[a], hi = end - 1;
            const double v = (std::trunc((*axes[a])[lo]) / scaling + std::trunc((*axes[a])[hi]) / scaling) * 0.5;
            tab.push_back(a == 2 ? (float)(-v) : (float)v);
        }
    for (uint32_t c = 0; c < 256; ++c) tab.push_back((float)((double)c / 255.0));
    VC_TRY(ensure(ctx, sh.tab, tab.size()));
    VC_TRY(ensure(ctx, sh.view, (size_t)sh.T * 6));
    VC_HIP(ctx, hipMemcpy(sh.tab.ptr, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    const ShGrid cg = shell_grid(nullptr, 0, sh.dims[0], sh.dims[1], sh.dims[2]);
    float *pos = sh.view.ptr, *col = pos + (size_t)sh.T * 3;
    hipLaunchKernelGGL(k_sh_viewer, dim3((uint32_t)((sh.T + kShBlock - 1) / kShBlock)), dim3(kShBlock), 0, ctx->stream,
                       (const uint64_t *)sh.rec.ptr, sh.T, cg, (const float *)sh.tab.ptr, pos, col);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (positions) VC_HIP(ctx, hipMemcpy(positions, pos, (size_t)sh.T * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (colors) VC_HIP(ctx, hipMemcpy(colors, col, (size_t)sh.T * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return VC_OK;
}
