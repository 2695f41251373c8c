// ---- lit renders: cast shadows, ambient occlusion and a floor for the last render (vc_light.h; contract in include/voxcarve.h) ----
// Reads the images of the last render, the occupancy words, the block map and the records (smooth = 1: the normals); writes its
// own images only.
int vc_light_render(vc_ctx *ctx, const vc_light_t *light, uint32_t flags, vc_light_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_light_render: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_light_render: flags must be 0 (got %u)", flags);
    if (!light) return fail(ctx, VC_ERR_ARG, "vc_light_render: no light");
    const vc_light_t &l = *light;
    for (int j = 0; j < 4; ++j)
        if (!std::isfinite(l.pos[j])) return fail(ctx, VC_ERR_ARG, "vc_light_render: the light has a component that is not finite");
    if (l.pos[3] != 0.0 && l.pos[3] != 1.0)
        return fail(ctx, VC_ERR_ARG, "vc_light_render: pos[3] = %g is neither 1 (a point in mm) nor 0 (a direction)", l.pos[3]);
    if (l.pos[3] == 0.0 && !std::isnormal((l.pos[0] * l.pos[0] + l.pos[1] * l.pos[1]) + l.pos[2] * l.pos[2]))
        return fail(ctx, VC_ERR_ARG, "vc_light_render: the light's direction has squared length %g",
                    (l.pos[0] * l.pos[0] + l.pos[1] * l.pos[1]) + l.pos[2] * l.pos[2]);
    if (l.ambient > 255) return fail(ctx, VC_ERR_ARG, "vc_light_render: ambient %u not in 0..255", l.ambient);
    if (l.smooth > 1) return fail(ctx, VC_ERR_ARG, "vc_light_render: smooth %u is neither 0 nor 1", l.smooth);
    if (!std::isfinite(l.ao_reach) || l.ao_reach < 0.0) return fail(ctx, VC_ERR_ARG, "vc_light_render: ao_reach %g is negative or not finite", l.ao_reach);
    if (l.floor > 1) return fail(ctx, VC_ERR_ARG, "vc_light_render: floor %u is neither 0 nor 1", l.floor);
    if (l.floor) {
        double big = 0.0;
        for (int j = 0; j < 4; ++j) {
            if (!std::isfinite(l.floor_rect[j])) return fail(ctx, VC_ERR_ARG, "vc_light_render: the floor's rectangle has a bound that is not finite");
            big = std::fabs(l.floor_rect[j]) > big ? std::fabs(l.floor_rect[j]) : big;
        }
        if (!std::isfinite(l.floor_z)) return fail(ctx, VC_ERR_ARG, "vc_light_render: floor_z is not finite");
        if (l.floor_rect[0] > l.floor_rect[1] || l.floor_rect[2] > l.floor_rect[3])
            return fail(ctx, VC_ERR_ARG, "vc_light_render: the floor's rectangle [%g, %g] x [%g, %g] is empty", l.floor_rect[0], l.floor_rect[1],
                        l.floor_rect[2], l.floor_rect[3]);
        // (the cells of a point of the rectangle are counted in 64-bit integers)
        if (!std::isfinite(l.floor_cell_mm) || !(l.floor_cell_mm > 0.0) || !(big / l.floor_cell_mm < 4503599627370496.0))
            return fail(ctx, VC_ERR_ARG, "vc_light_render: floor cells of %g mm (must be > 0 and at most 2^52 of them to the rectangle's bounds)",
                        l.floor_cell_mm);
    }
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_light_render", "light", "lighting", pass));
    if (!ctx->render.valid || !ctx->current(ctx->render.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_light_render: no images of the current carve result: call vc_render first");
    if (l.smooth && !ctx->current(ctx->normals.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_light_render: smooth = 1 and no normals: call vc_hull_normals on the current carve result");
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    VC_HIP(ctx, ensure_pinned(ctx->light.h, 7));
    ctx->light.valid = false;
    const uint32_t V = ctx->render.n_views, H = ctx->render.H, W = ctx->render.W;
    const uint64_t npix = (uint64_t)V * H * W;                           // <= 2^28 (vc_render)
    VC_TRY(ensure(ctx, ctx->light.rgb, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->light.jobs, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->light.depth, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->light.kind, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->light.shadow, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->light.ao, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->light.ctr, 7));
    const uint32_t nb[3] = {(ctx->nx + kRenderB - 1) / kRenderB, (ctx->ny + kRenderB - 1) / kRenderB, (ctx->nz + kRenderB - 1) / kRenderB};
    const uint64_t nblocks = (uint64_t)nb[0] * nb[1] * nb[2];
    VC_TRY(ensure(ctx, ctx->render.map, (size_t)((nblocks + 63) / 64)));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    VC_HIP(ctx, hipMemsetAsync(ctx->light.ctr.ptr, 0, 7 * sizeof(unsigned long long), ctx->stream));
    LightParams p;
    memset(&p, 0, sizeof p);
    p.words = cur.words.ptr;
    p.bmap = ctx->render.map.ptr;
    p.records = cur.records.ptr;
    p.normals = ctx->normals.out.ptr;
    p.S = ctx->survivors;
    p.views = ctx->render.views.ptr;
    p.idx = ctx->render.idx.ptr; p.depth = ctx->render.depth.ptr; p.rgbf = ctx->render.rgbf.ptr;
    p.jobs = ctx->light.jobs.ptr;
    p.rgb = ctx->light.rgb.ptr; p.odepth = ctx->light.depth.ptr;
    p.kind = ctx->light.kind.ptr; p.shadow = ctx->light.shadow.ptr; p.ao = ctx->light.ao.ptr;
    p.ctr = ctx->light.ctr.ptr;
    const uint32_t n3[3] = {ctx->nx, ctx->ny, ctx->nz};
    for (int a = 0; a < 3; ++a) {                // item 1 of vc_render
        p.n[a] = n3[a];
        p.nb[a] = nb[a];
        p.s[a] = (ctx->bounds[2 * a + 1] - ctx->bounds[2 * a]) / (double)(n3[a] - 1);
        p.e[a] = ctx->bounds[2 * a] - 0.5 * p.s[a];
    }
    p.H = H; p.W = W; p.npix = (uint32_t)npix;
    p.skip = ctx->render.blocks ? 1u : 0u;
    for (int j = 0; j < 4; ++j) { p.pos[j] = l.pos[j]; p.rect[j] = l.floor_rect[j]; }
    p.ambient = l.ambient; p.smooth = l.smooth; p.floor = l.floor;
    p.ao_reach = l.ao_reach; p.floor_z = l.floor_z; p.cell = l.floor_cell_mm;
    for (int k = 0; k < 2; ++k)
        p.floor_rgb[k] = (uint32_t)l.floor_rgb[k][0] | ((uint32_t)l.floor_rgb[k][1] << 8) | ((uint32_t)l.floor_rgb[k][2] << 16);
    if (p.skip && !ctx->render.map_built) {       // (render_blocks was 0 when the render ran: the map of the same result, now)
        hipLaunchKernelGGL(k_render_map, dim3((uint32_t)((nblocks + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0, ctx->stream,
                           (const uint64_t *)cur.words.ptr, ctx->render.map.ptr, ctx->nx, ctx->ny, ctx->nz, nb[0], nb[1], nblocks);
        VC_HIP(ctx, hipGetLastError());
        ctx->render.map_built = true;
    }
    hipLaunchKernelGGL(k_light_classify, dim3((uint32_t)((npix + kLightBlock - 1) / kLightBlock)), dim3(kLightBlock), 0, ctx->stream, p);
    VC_HIP(ctx, hipGetLastError());
    const LightSel sel{ctx->light.kind.ptr, ctx->render.rgbf.ptr, ctx->light.jobs.ptr};
    VC_TRY(compact(ctx, sel, npix, ctx->h_res + 0));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));                  // the list's length sizes the launch
    const uint64_t njobs = ctx->h_res[0];
    if (njobs > npix) return fail(ctx, VC_ERR_HIP, "vc_light_render: %llu pixels listed among %llu", (unsigned long long)njobs, (unsigned long long)npix);
    p.njobs = (uint32_t)njobs;
    if (njobs) {
        const uint64_t per = kLightBlock / kLightRays, want = (njobs + per - 1) / per;
        hipLaunchKernelGGL(k_light, dim3((uint32_t)(want < kLightMaxBlocks ? want : kLightMaxBlocks)), dim3(kLightBlock), 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
    }
    VC_TRY(pass_stop(ctx, pass));                   // (the counters' read-back is not part of the pass's time)
    VC_HIP(ctx, hipMemcpyAsync(ctx->light.h, ctx->light.ctr.ptr, 7 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->light_ms));
    const uint64_t *h = ctx->light.h;
    if (h[0] + h[1] > npix || njobs > h[0] + h[1] || h[2] + h[3] > njobs)
        return fail(ctx, VC_ERR_HIP, "vc_light_render: %llu hull and %llu floor pixels among %llu, %llu listed, %llu shadowed, %llu facing away",
                    (unsigned long long)h[0], (unsigned long long)h[1], (unsigned long long)npix, (unsigned long long)njobs,
                    (unsigned long long)h[2], (unsigned long long)h[3]);
    ctx->light.valid = true;
    stats->pixels = npix;
    stats->hull_pixels = h[0];
    stats->floor_pixels = h[1];
    stats->shadowed = h[2];
    stats->facing_away = h[3];
    stats->rays_walked = h[4];
    stats->cells_visited = h[5];
    stats->blocks_skipped = h[6];
    return VC_OK;
}

int vc_fetch_lit(vc_ctx *ctx, uint32_t view, uint8_t *rgb, float *depth, uint8_t *kind, uint8_t *shadow, uint8_t *ao)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->render.valid || !ctx->light.valid) return fail(ctx, VC_ERR_ARG, "vc_fetch_lit: no lit images: call vc_light_render first");
    if (view >= ctx->render.n_views) return fail(ctx, VC_ERR_ARG, "vc_fetch_lit: view %u not in [0,%u)", view, ctx->render.n_views);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)ctx->render.H * ctx->render.W, off = (size_t)view * HW;
    if (rgb) {
        std::vector<uint32_t> px(HW);
        VC_HIP(ctx, hipMemcpy(px.data(), ctx->light.rgb.ptr + off, HW * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < HW; ++k) {
            const uint32_t q = px[k];
            rgb[3 * k] = (uint8_t)q; rgb[3 * k + 1] = (uint8_t)(q >> 8); rgb[3 * k + 2] = (uint8_t)(q >> 16);
        }
    }
    if (depth) VC_HIP(ctx, hipMemcpy(depth, ctx->light.depth.ptr + off, HW * sizeof(float), hipMemcpyDeviceToHost));
    if (kind) VC_HIP(ctx, hipMemcpy(kind, ctx->light.kind.ptr + off, HW, hipMemcpyDeviceToHost));
    if (shadow) VC_HIP(ctx, hipMemcpy(shadow, ctx->light.shadow.ptr + off, HW, hipMemcpyDeviceToHost));
    if (ao) VC_HIP(ctx, hipMemcpy(ao, ctx->light.ao.ptr + off, HW, hipMemcpyDeviceToHost));
    return VC_OK;
}
