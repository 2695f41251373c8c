// ---- surface normals of the current carve result, shaded renders, mesh normals (vc_normals.h; contract in include/voxcarve.h) ----
int vc_hull_normals(vc_ctx *ctx, uint64_t r2, uint32_t flags, vc_normals_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_normals: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_hull_normals: flags must be 0 (got %u)", flags);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_normals", "give normals to", "normal estimation", pass));
    uint64_t q[3];
    VC_TRY(dist_metric(ctx, "vc_hull_normals", q));
    // item 2: the ball's extents and its rows (dx, dz) with their y half-extent
    const uint64_t root = isqrt_u64(r2);
    uint32_t ext[3];
    for (int a = 0; a < 3; ++a) {
        const uint64_t e = root / q[a];
        if (e > kNrmMaxExt)
            return fail(ctx, VC_ERR_ARG, "vc_hull_normals: r2 = %llu um^2 reaches %llu cells along %c, more than %u", (unsigned long long)r2,
                        (unsigned long long)e, "xyz"[a], kNrmMaxExt);
        ext[a] = (uint32_t)e;
    }
    if (!(ext[0] | ext[1] | ext[2])) return fail(ctx, VC_ERR_ARG, "vc_hull_normals: the ball of r2 = %llu um^2 holds no voxel offset", (unsigned long long)r2);
    std::vector<uint32_t> rows;
    uint64_t offsets = 0;
    for (int32_t dz = -(int32_t)ext[2]; dz <= (int32_t)ext[2]; ++dz)
        for (int32_t dx = -(int32_t)ext[0]; dx <= (int32_t)ext[0]; ++dx) {
            const uint64_t used = (q[0] * (uint64_t)std::abs(dx)) * (q[0] * (uint64_t)std::abs(dx)) +
                                  (q[2] * (uint64_t)std::abs(dz)) * (q[2] * (uint64_t)std::abs(dz));
            if (used > r2) continue;
            const uint32_t ky = (uint32_t)(isqrt_u64(r2 - used) / q[1]);         // <= ext[1]
            if (ky == 0 && dx == 0 && dz == 0) continue;                          // the voxel itself alone
            rows.push_back(((uint32_t)dx & 255u) | (((uint32_t)dz & 255u) << 8) | (ky << 16));
            offsets += 2ull * ky + ((dx == 0 && dz == 0) ? 0u : 1u);
        }
    const uint64_t S = pass.S, n = pass.n, nwords = pass.nwords;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_normals: %llu voxels exceed the u32 index", (unsigned long long)n);
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->normals.stamp = kNever;
    if (S) {
        VC_TRY(ensure(ctx, ctx->d_rscan, word_groups(nwords)));
        VC_TRY(ensure(ctx, ctx->d_woff, (size_t)nwords));
        VC_TRY(ensure(ctx, ctx->normals.rows, rows.size()));
        VC_TRY(ensure(ctx, ctx->normals.out, (size_t)S));
        VC_TRY(ensure(ctx, ctx->normals.ctr, 2));
    }
    VC_TRY(pass_start(ctx, pass));
    ctx->h_res[0] = ctx->h_res[1] = 0;
    if (S) {
        VC_HIP(ctx, hipMemcpyAsync(ctx->normals.rows.ptr, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(ctx->normals.out.ptr, 0, (size_t)S * sizeof(short4), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(ctx->normals.ctr.ptr, 0, 2 * sizeof(unsigned long long), ctx->stream));
        VC_TRY(word_offsets(ctx, cur, nwords, ctx->d_woff, ctx->h_res + 2));
        NrmParams p;
        memset(&p, 0, sizeof p);
        p.words = cur.words.ptr; p.woff = ctx->d_woff.ptr; p.rows = ctx->normals.rows.ptr;
        p.out = ctx->normals.out.ptr; p.ctr = ctx->normals.ctr.ptr;
        p.nwords = nwords; p.n = n; p.S = S;
        for (int a = 0; a < 3; ++a) p.q[a] = (long long)q[a];
        p.nrows = (uint32_t)rows.size(); p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz;
        const uint64_t per_block = (uint64_t)(kNrmBlock / 64) * kNrmWords;
        hipLaunchKernelGGL(k_normals, dim3((uint32_t)((nwords + per_block - 1) / per_block)), dim3(kNrmBlock), 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(ctx->h_res, ctx->normals.ctr.ptr, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    VC_TRY(pass_end(ctx, pass, &stats->normals_ms));
    if (S && ctx->h_res[2] != S)
        return fail(ctx, VC_ERR_HIP, "vc_hull_normals: the occupancy holds %llu voxels, the result %llu records", (unsigned long long)ctx->h_res[2],
                    (unsigned long long)S);
    if (ctx->h_res[0] > S || ctx->h_res[1] > ctx->h_res[0])
        return fail(ctx, VC_ERR_HIP, "vc_hull_normals: %llu surface records, %llu of them without a normal, among %llu", (unsigned long long)ctx->h_res[0],
                    (unsigned long long)ctx->h_res[1], (unsigned long long)S);
    stats->survivors = S;
    stats->surface = ctx->h_res[0];
    stats->zero = ctx->h_res[1];
    stats->offsets = offsets;
    for (int a = 0; a < 3; ++a) { stats->q[a] = q[a]; stats->ext[a] = ext[a]; }
    ctx->normals.stamp = ctx->result_gen;
    ctx->normals.n = S;
    return VC_OK;
}

int vc_fetch_record_normals(vc_ctx *ctx, int16_t *n4)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->normals.stamp)) return fail(ctx, VC_ERR_ARG, "no normals: call vc_hull_normals on the current carve result");
    if (!n4) return VC_OK;                       // only asked whether the normals are valid
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->normals.n) VC_HIP(ctx, hipMemcpy(n4, ctx->normals.out.ptr, (size_t)ctx->normals.n * sizeof(short4), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_shade_render(vc_ctx *ctx, const double *light, uint32_t ambient, uint32_t flags)
{
    if (!ctx) return VC_ERR_ARG;
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_shade_render: flags must be 0 (got %u)", flags);
    if (!light) return fail(ctx, VC_ERR_ARG, "vc_shade_render: no lights");
    if (ambient > 255) return fail(ctx, VC_ERR_ARG, "vc_shade_render: ambient %u not in 0..255", ambient);
    if (!ctx->carved || !ctx->current(ctx->normals.stamp)) return fail(ctx, VC_ERR_ARG, "vc_shade_render: no normals: call vc_hull_normals on the current carve result");
    if (!ctx->render.valid || !ctx->current(ctx->render.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_shade_render: no images of the current carve result: call vc_render first");
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    for (uint32_t v = 0; v < ctx->render.n_views; ++v) {
        const double *L = light + 3 * (size_t)v;
        if (!std::isfinite(L[0]) || !std::isfinite(L[1]) || !std::isfinite(L[2]))
            return fail(ctx, VC_ERR_ARG, "vc_shade_render: the light of view %u has a component that is not finite", v);
        const double ll = (L[0] * L[0] + L[1] * L[1]) + L[2] * L[2];
        if (!std::isnormal(ll)) return fail(ctx, VC_ERR_ARG, "vc_shade_render: the light of view %u has squared length %g", v, ll);
    }
    StepBuf &cur = ctx->sb[ctx->cur];
    VC_HIP(ctx, hipSetDevice(ctx->device));
    ctx->normals.sh_valid = false;
    const uint64_t view_pix = (uint64_t)ctx->render.H * ctx->render.W, npix = view_pix * ctx->render.n_views;
    VC_TRY(ensure(ctx, ctx->normals.sh_rgb, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->normals.sh_light, 3 * (size_t)ctx->render.n_views));
    VC_HIP(ctx, hipMemcpyAsync(ctx->normals.sh_light.ptr, light, 3 * (size_t)ctx->render.n_views * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ShadeParams p;
    memset(&p, 0, sizeof p);
    p.idx = ctx->render.idx.ptr; p.rgbf = ctx->render.rgbf.ptr;
    p.records = cur.records.ptr; p.normals = ctx->normals.out.ptr; p.light = ctx->normals.sh_light.ptr;
    p.out = ctx->normals.sh_rgb.ptr;
    p.S = ctx->survivors; p.npix = npix; p.view_pix = view_pix; p.ambient = ambient;
    hipLaunchKernelGGL(k_shade, dim3((uint32_t)((npix + kNrmBlock - 1) / kNrmBlock)), dim3(kNrmBlock), 0, ctx->stream, p);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));             // (the lights are the caller's memory)
    ctx->normals.sh_valid = true;
    return VC_OK;
}

int vc_fetch_shaded(vc_ctx *ctx, uint32_t view, uint8_t *rgb)
{
    if (!ctx || !rgb) return VC_ERR_ARG;
    if (!ctx->render.valid || !ctx->normals.sh_valid) return fail(ctx, VC_ERR_ARG, "vc_fetch_shaded: no shaded images: call vc_shade_render first");
    if (view >= ctx->render.n_views) return fail(ctx, VC_ERR_ARG, "vc_fetch_shaded: view %u not in [0,%u)", view, ctx->render.n_views);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)ctx->render.H * ctx->render.W, off = (size_t)view * HW;
    std::vector<uint32_t> px(HW);
    VC_HIP(ctx, hipMemcpy(px.data(), ctx->normals.sh_rgb.ptr + off, HW * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < HW; ++k) {
        const uint32_t q = px[k];
        rgb[3 * k] = (uint8_t)q; rgb[3 * k + 1] = (uint8_t)(q >> 8); rgb[3 * k + 2] = (uint8_t)(q >> 16);
    }
    return VC_OK;
}

int vc_surface_normals(vc_ctx *ctx, int16_t *n4)
{
    if (!ctx || !n4) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->normals.stamp)) return fail(ctx, VC_ERR_ARG, "vc_surface_normals: no normals: call vc_hull_normals on the current carve result");
    if (!ctx->surface.valid || !ctx->current(ctx->surface.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_surface_normals: no mesh of the current carve result: call vc_surface_mesh first");
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    const uint64_t V = ctx->surface.n_verts;
    if (!V) return VC_OK;
    StepBuf &cur = ctx->sb[ctx->cur];
    VC_HIP(ctx, hipSetDevice(ctx->device));
    VC_TRY(ensure(ctx, ctx->normals.verts, (size_t)V));
    hipLaunchKernelGGL(k_surf_normals, dim3((uint32_t)((V + kNrmBlock - 1) / kNrmBlock)), dim3(kNrmBlock), 0, ctx->stream,
                       (const uint64_t *)ctx->surface.edges.ptr, V, (const uint64_t *)cur.records.ptr, ctx->survivors,
                       (const short4 *)ctx->normals.out.ptr, ctx->nx, ctx->ny, ctx->normals.verts.ptr);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipMemcpyAsync(n4, ctx->normals.verts.ptr, (size_t)V * sizeof(short4), hipMemcpyDeviceToHost, ctx->stream));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VC_OK;
}
