// ---- free-viewpoint texturing of the last render (vc_texture.h; contract in include/voxcarve.h) ----
// Reads the images of the last render, the carve's masks and threshold, the depth maps of the current vc_color_visible and the
// images of `slot`; writes its own images only.
int vc_texture_render(vc_ctx *ctx, uint32_t slot, uint32_t steps, double reach_mm, float depth_tolerance, uint32_t best,
                      uint32_t sharpen, uint32_t filter, uint32_t flags, vc_texture_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_texture_render: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_texture_render: flags must be 0 (got %u)", flags);
    if (steps > kTexMaxSteps) return fail(ctx, VC_ERR_ARG, "vc_texture_render: steps %u not in [0, %u]", steps, kTexMaxSteps);
    if (!std::isfinite(reach_mm) || reach_mm < 0.0) return fail(ctx, VC_ERR_ARG, "vc_texture_render: reach %g mm is negative or not finite", reach_mm);
    if (!std::isfinite(depth_tolerance) || depth_tolerance < 0.0f)
        return fail(ctx, VC_ERR_ARG, "vc_texture_render: depth tolerance %g is negative or not finite", (double)depth_tolerance);
    if (best < 1 || best > VC_MAX_CAMERAS) return fail(ctx, VC_ERR_ARG, "vc_texture_render: best %u not in [1, %d]", best, VC_MAX_CAMERAS);
    if (sharpen > kTexMaxSharpen) return fail(ctx, VC_ERR_ARG, "vc_texture_render: sharpen %u not in [0, %u]", sharpen, kTexMaxSharpen);
    if (filter > 1) return fail(ctx, VC_ERR_ARG, "vc_texture_render: filter %u is neither 0 (nearest) nor 1 (bilinear)", filter);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_texture_render", "texture", "texturing", pass));
    if (!ctx->render.valid || !ctx->current(ctx->render.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_texture_render: no images of the current carve result: call vc_render first");
    if (!ctx->current(ctx->visible.stamp))
        return fail(ctx, VC_ERR_ARG, "vc_texture_render: no depth maps of the current carve result: call vc_color_visible first");
    if (slot >= ctx->slots.size() || !ctx->slots[slot].have_masks) return fail(ctx, VC_ERR_ARG, "vc_texture_render: no frame set in slot %u", slot);
    Slot &s = ctx->slots[slot];
    for (uint32_t c = 0; c < ctx->C; ++c)
        if (c >= s.have_frame.size() || !s.have_frame[c]) return fail(ctx, VC_ERR_ARG, "vc_texture_render: camera %u has no frame in slot %u", c, slot);
    StepBuf &cur = *pass.cur;
    // the point test reads the masks the occupancy came from (vc_surface_mesh's rule); bringing new images of the carve's own frame
    // set into the record layout below would prepare it again
    if (steps > 0 && (cur.slot >= ctx->slots.size() || ctx->slots[cur.slot].gen != cur.slot_gen || (slot == cur.slot && !s.bits_valid)))
        return fail(ctx, VC_ERR_ARG, "vc_texture_render: frame set %u has been prepared again since the carve, or has masks or images that "
                    "wait for it: its masks are not the ones the occupancy came from (steps = 0 needs no masks)", cur.slot);
    VC_TRY(pass_begin(ctx));
    VC_HIP(ctx, ensure_pinned(ctx->texture.h, 5));
    ctx->texture.valid = false;
    const uint32_t V = ctx->render.n_views, H = ctx->render.H, W = ctx->render.W;
    const uint64_t npix = (uint64_t)V * H * W;
    VC_TRY(ensure(ctx, ctx->texture.rgbc, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->texture.depth, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->texture.best, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->texture.refined, (size_t)npix));
    VC_TRY(ensure(ctx, ctx->texture.ctr, 5));
    VC_TRY(visible_start(ctx, s, pass));            // the slot's images in the record layout; the occupancy words are not read
    VC_HIP(ctx, hipMemsetAsync(ctx->texture.ctr.ptr, 0, 5 * sizeof(unsigned long long), ctx->stream));
    TexParams p;
    memset(&p, 0, sizeof p);
    p.views = ctx->render.views.ptr;
    p.idx = ctx->render.idx.ptr; p.depth = ctx->render.depth.ptr; p.rgbf = ctx->render.rgbf.ptr;
    p.zmap = ctx->visible.zmap.ptr;
    p.frames = s.frames.ptr;
    p.bits = ctx->slots[cur.slot].bits.ptr;
    p.rgbc = ctx->texture.rgbc.ptr; p.odepth = ctx->texture.depth.ptr; p.best = ctx->texture.best.ptr; p.refined = ctx->texture.refined.ptr;
    p.ctr = ctx->texture.ctr.ptr;
    p.H = H; p.W = W;
    p.tiles_x = (W + 7) / 8;
    p.tiles_per_view = p.tiles_x * ((H + 7) / 8);
    p.n_tiles = p.tiles_per_view * V;
    p.C = ctx->C; p.CH = ctx->H; p.CW = ctx->W; p.mwords = ctx->mwords;
    p.m = cur.min_views; p.steps = steps; p.keep = best; p.sharpen = sharpen; p.filter = filter;
    p.tol = depth_tolerance;
    p.reach = reach_mm;
    memcpy(p.cam, ctx->cams, sizeof(CamDev) * ctx->C);
    for (uint32_t c = 0; c < ctx->C; ++c) {          // item 5: a camera's centre, as the render makes a view's origin
        const double *R = ctx->cams[c].r, *t = ctx->cams[c].t;
        for (int j = 0; j < 3; ++j) p.centre[c][j] = -((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]);
    }
    hipLaunchKernelGGL(k_texture, dim3((p.n_tiles + kTexBlock / 64 - 1) / (kTexBlock / 64)), dim3(kTexBlock), 0, ctx->stream, p);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(pass_stop(ctx, pass));                   // (the counters' read-back is not part of the pass's time)
    VC_HIP(ctx, hipMemcpyAsync(ctx->texture.h, ctx->texture.ctr.ptr, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->texture_ms));
    const uint64_t *h = ctx->texture.h;
    if (h[0] > npix || h[1] > h[0] || h[2] + h[3] != h[0])
        return fail(ctx, VC_ERR_HIP, "vc_texture_render: %llu hits among %llu pixels, %llu refined, %llu textured, %llu fallback",
                    (unsigned long long)h[0], (unsigned long long)npix, (unsigned long long)h[1], (unsigned long long)h[2], (unsigned long long)h[3]);
    ctx->texture.valid = true;
    stats->pixels = npix;
    stats->hits = h[0];
    stats->refined = h[1];
    stats->textured = h[2];
    stats->fallback = h[3];
    stats->point_tests = h[4];
    return VC_OK;
}

int vc_fetch_textured(vc_ctx *ctx, uint32_t view, uint8_t *rgb, float *depth, uint8_t *count, uint8_t *best_cam, uint8_t *refined)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->render.valid || !ctx->texture.valid) return fail(ctx, VC_ERR_ARG, "vc_fetch_textured: no textured images: call vc_texture_render first");
    if (view >= ctx->render.n_views) return fail(ctx, VC_ERR_ARG, "vc_fetch_textured: view %u not in [0,%u)", view, ctx->render.n_views);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t HW = (size_t)ctx->render.H * ctx->render.W, off = (size_t)view * HW;
    if (rgb || count) {
        std::vector<uint32_t> px(HW);
        VC_HIP(ctx, hipMemcpy(px.data(), ctx->texture.rgbc.ptr + off, HW * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < HW; ++k) {
            const uint32_t q = px[k];
            if (rgb) { rgb[3 * k] = (uint8_t)q; rgb[3 * k + 1] = (uint8_t)(q >> 8); rgb[3 * k + 2] = (uint8_t)(q >> 16); }
            if (count) count[k] = (uint8_t)(q >> 24);
        }
    }
    if (depth) VC_HIP(ctx, hipMemcpy(depth, ctx->texture.depth.ptr + off, HW * sizeof(float), hipMemcpyDeviceToHost));
    if (best_cam) VC_HIP(ctx, hipMemcpy(best_cam, ctx->texture.best.ptr + off, HW, hipMemcpyDeviceToHost));
    if (refined) VC_HIP(ctx, hipMemcpy(refined, ctx->texture.refined.ptr + off, HW, hipMemcpyDeviceToHost));
    return VC_OK;
}
