// ---- ray-cast images of the current carve result (vc_render.h; contract in include/voxcarve.h) ----
int vc_render(vc_ctx *ctx, uint32_t n_views, const vc_view_t *views, uint32_t H, uint32_t W, const uint8_t *shade,
              const uint8_t *background, uint32_t flags, vc_render_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (stats) memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_render: flags must be 0 (got %u)", flags);
    if (n_views == 0 || !views) return fail(ctx, VC_ERR_ARG, "vc_render: no views");
    if (H < 1 || H > 16384 || W < 1 || W > 16384) return fail(ctx, VC_ERR_ARG, "vc_render: image size %ux%u not in 1..16384", H, W);
    const uint64_t npix = (uint64_t)n_views * H * W;
    if (npix > (1ull << 28)) return fail(ctx, VC_ERR_ARG, "vc_render: %u views of %ux%u are %llu pixels, more than 2^28", n_views, H, W,
                                         (unsigned long long)npix);
    for (uint32_t k = 0; k < n_views; ++k) {
        const double *q = views[k].K;                               // the 21 doubles of the view
        for (int j = 0; j < 21; ++j)
            if (!std::isfinite(q[j])) return fail(ctx, VC_ERR_ARG, "vc_render: view %u has a parameter that is not finite", k);
        if (!(views[k].K[0] > 0.0) || !(views[k].K[1] > 0.0))
            return fail(ctx, VC_ERR_ARG, "vc_render: view %u has fx %g, fy %g (both must be > 0)", k, views[k].K[0], views[k].K[1]);
    }
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_render", "render", "rendering", pass));
    if (ctx->nx < 2 || ctx->ny < 2 || ctx->nz < 2)
        return fail(ctx, VC_ERR_ARG, "vc_render: grid %ux%ux%u has an axis shorter than 2", ctx->nx, ctx->ny, ctx->nz);
    static_assert(sizeof(vc_view_t) == sizeof(RenderView), "vc_view_t is the device's view");
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->render.valid = false; ctx->render.stamp = kNever; ctx->normals.sh_valid = false; ctx->texture.valid = false;
    ctx->light.valid = false; ctx->render.map_built = false;
    VC_TRY(ensure(ctx, ctx->render.idx, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->render.depth, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->render.rgbf, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->render.views, n_views));
    VC_TRY(ensure(ctx, ctx->render.ctr, 3));
    const uint32_t nb[3] = {(ctx->nx + kRenderB - 1) / kRenderB, (ctx->ny + kRenderB - 1) / kRenderB, (ctx->nz + kRenderB - 1) / kRenderB};
    const uint64_t nblocks = (uint64_t)nb[0] * nb[1] * nb[2];
    VC_TRY(ensure(ctx, ctx->render.map, (size_t)((nblocks + 63) / 64)));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    VC_HIP(ctx, hipMemcpyAsync(ctx->render.views.ptr, views, (size_t)n_views * sizeof(vc_view_t), hipMemcpyHostToDevice, ctx->stream));
    VC_HIP(ctx, hipMemsetAsync(ctx->render.ctr.ptr, 0, 3 * sizeof(unsigned long long), ctx->stream));
    RenderParams p;
    memset(&p, 0, sizeof p);
    p.words = cur.words.ptr;
    p.bmap = ctx->render.map.ptr;
    p.records = cur.records.ptr;
    p.S = ctx->survivors;
    p.views = ctx->render.views.ptr;
    p.idx = ctx->render.idx.ptr; p.depth = ctx->render.depth.ptr; p.rgbf = ctx->render.rgbf.ptr;
    p.ctr = ctx->render.ctr.ptr;
    const uint32_t n3[3] = {ctx->nx, ctx->ny, ctx->nz};
    for (int a = 0; a < 3; ++a) {                // item 1 (this file is built without contraction too)
        p.n[a] = n3[a];
        p.nb[a] = nb[a];
        p.s[a] = (ctx->bounds[2 * a + 1] - ctx->bounds[2 * a]) / (double)(n3[a] - 1);
        p.e[a] = ctx->bounds[2 * a] - 0.5 * p.s[a];
    }
    p.H = H; p.W = W;
    p.tiles_x = (W + 7) / 8;
    p.tiles_per_view = p.tiles_x * ((H + 7) / 8);
    p.n_tiles = p.tiles_per_view * n_views;      // <= 2^28 views x tiles of one pixel
    for (int f = 0; f < 7; ++f) p.shade[f] = shade ? shade[f] : 255u;
    p.bg = background ? (uint32_t)background[0] | ((uint32_t)background[1] << 8) | ((uint32_t)background[2] << 16) : 0u;
    p.skip = ctx->render.blocks ? 1u : 0u;
    if (p.skip) {
        hipLaunchKernelGGL(k_render_map, dim3((uint32_t)((nblocks + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0, ctx->stream,
                           (const uint64_t *)cur.words.ptr, ctx->render.map.ptr, ctx->nx, ctx->ny, ctx->nz, nb[0], nb[1], nblocks);
        VC_HIP(ctx, hipGetLastError());
        ctx->render.map_built = true;
    }
    hipLaunchKernelGGL(k_render, dim3((p.n_tiles + kRenderBlock / 64 - 1) / (kRenderBlock / 64)), dim3(kRenderBlock), 0, ctx->stream, p);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(pass_stop(ctx, pass));                   // (the counters' read-back is not part of the render's time)
    VC_HIP(ctx, hipMemcpyAsync(ctx->h_res, ctx->render.ctr.ptr, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, stats ? &stats->render_ms : nullptr));
    ctx->render.valid = true; ctx->render.stamp = ctx->result_gen;
    ctx->render.n_views = n_views; ctx->render.H = H; ctx->render.W = W;
    if (ctx->h_res[0] > npix) return fail(ctx, VC_ERR_HIP, "vc_render: %llu hits among %llu pixels", (unsigned long long)ctx->h_res[0],
                                          (unsigned long long)npix);
    if (stats) {
        stats->pixels = npix;
        stats->hits = ctx->h_res[0];
        stats->cells_visited = ctx->h_res[1];
        stats->blocks_skipped = ctx->h_res[2];
    }
    return VC_OK;
}

int vc_fetch_render(vc_ctx *ctx, uint32_t view, uint32_t *idx, float *depth, uint8_t *rgb, uint8_t *face)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->render.valid) return fail(ctx, VC_ERR_ARG, "vc_fetch_render: no images: call vc_render first");
    if (view >= ctx->render.n_views) return fail(ctx, VC_ERR_ARG, "vc_fetch_render: view %u not in [0,%u)", view, ctx->render.n_views);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)ctx->render.H * ctx->render.W, off = (size_t)view * HW;
    if (idx) VC_HIP(ctx, hipMemcpy(idx, ctx->render.idx.ptr + off, HW * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (depth) VC_HIP(ctx, hipMemcpy(depth, ctx->render.depth.ptr + off, HW * sizeof(float), hipMemcpyDeviceToHost));
    if (rgb || face) {
        std::vector<uint32_t> px(HW);
        VC_HIP(ctx, hipMemcpy(px.data(), ctx->render.rgbf.ptr + off, HW * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < HW; ++k) {
            const uint32_t q = px[k];
            if (rgb) { rgb[3 * k] = (uint8_t)q; rgb[3 * k + 1] = (uint8_t)(q >> 8); rgb[3 * k + 2] = (uint8_t)(q >> 16); }
            if (face) face[k] = (uint8_t)(q >> 24);
        }
    }
    return VC_OK;
}

int vc_fetch_visibility(vc_ctx *ctx, uint16_t *vis)
{
    if (!ctx || !vis) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->visible.stamp)) return fail(ctx, VC_ERR_ARG, "no visibility: call vc_color_visible on the current carve result");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->survivors) VC_HIP(ctx, hipMemcpy(vis, ctx->visible.mask.ptr, ctx->survivors * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_depth(vc_ctx *ctx, uint32_t cam, float *out)
{
    if (!ctx || !out) return VC_ERR_ARG;
    if (!ctx->carved || !ctx->current(ctx->visible.stamp)) return fail(ctx, VC_ERR_ARG, "no depth maps: call vc_color_visible on the current carve result");
    if (cam >= ctx->C) return fail(ctx, VC_ERR_ARG, "camera %u not in [0,%u)", cam, ctx->C);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)ctx->H * ctx->W;
    VC_HIP(ctx, hipMemcpy(out, ctx->visible.zmap.ptr + (size_t)cam * HW, HW * sizeof(float), hipMemcpyDeviceToHost));
    return VC_OK;
}
