// ---- silhouette-refined surface mesh of the current carve result (vc_surface.h; contract in include/voxcarve.h) ----
int vc_surface_mesh(vc_ctx *ctx, uint32_t steps, uint32_t flags, vc_surface_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    ctx->surface.valid = false; ctx->surface.stamp = kNever;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_surface_mesh: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags != 0) return fail(ctx, VC_ERR_ARG, "vc_surface_mesh: flags must be 0 (got %u)", flags);
    if (steps > kSurfMaxSteps) return fail(ctx, VC_ERR_ARG, "vc_surface_mesh: steps %u not in [0, %u]", steps, kSurfMaxSteps);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_surface_mesh", "colour the mesh from", "meshing", pass));
    StepBuf &cur = *pass.cur;
    if (cur.slot >= ctx->slots.size() || ctx->slots[cur.slot].gen != cur.slot_gen)
        return fail(ctx, VC_ERR_ARG, "vc_surface_mesh: frame set %u has been prepared again since the carve: its masks are not the ones "
                    "the occupancy came from", cur.slot);
    const uint64_t n = pass.n;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_surface_mesh: %llu voxels exceed the u32 index", (unsigned long long)n);
    const Slot &s = ctx->slots[cur.slot];
    VC_TRY(pass_begin(ctx));
    VC_TRY(pass_start(ctx, pass, kWordsAlways));
    uint64_t V = 0, F = 0;
    McParams p;
    memset(&p, 0, sizeof p);
    if (n) {
        // 1 topology: vc_marching_cubes(NULL, nz, nx, ny)'s counts and scans (its scratch, not its mesh)
        const uint32_t nwords = (uint32_t)((n + 63) / 64), ngroups = (nwords + 63) / 64;
        VC_TRY(ensure(ctx, ctx->d_mcx, (size_t)nwords * 3));
        VC_TRY(ensure(ctx, ctx->d_mcwbase, (size_t)nwords));
        VC_TRY(ensure(ctx, ctx->d_mcv, ngroups));
        VC_TRY(ensure(ctx, ctx->d_mct, ngroups));
        p.bits = cur.words.ptr;
        p.n = n; p.d0 = ctx->nz; p.d1 = ctx->nx; p.d2 = ctx->ny; p.nwords = nwords; p.ngroups = ngroups;
        p.x = ctx->d_mcx.ptr; p.wbase = ctx->d_mcwbase.ptr; p.gv = ctx->d_mcv.cnt.ptr; p.gt = ctx->d_mct.cnt.ptr;
        p.gvoff = ctx->d_mcv.off.ptr; p.gtoff = ctx->d_mct.off.ptr; p.bvoff = ctx->d_mcv.boff.ptr; p.btoff = ctx->d_mct.boff.ptr;
        hipLaunchKernelGGL(k_mc_count, dim3((ngroups + 3) / 4), dim3(kBlock), 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
        VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_mcv, ctx->d_mcv.cnt.ptr, ngroups, ctx->h_res));
        VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_mct, ctx->d_mct.cnt.ptr, ngroups, ctx->h_res + 1));
        // the one read-back in the middle: the counts size the mesh
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        V = ctx->h_res[0]; F = ctx->h_res[1];
        if (V > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_surface_mesh: %llu vertices exceed the u32 vertex number", (unsigned long long)V);
    }
    VC_TRY(ensure(ctx, ctx->surface.edges, (size_t)(V + 1)));
    VC_TRY(ensure(ctx, ctx->surface.verts, (size_t)(3 * V + 3)));
    VC_TRY(ensure(ctx, ctx->surface.faces, (size_t)(3 * F + 3)));
    VC_TRY(ensure(ctx, ctx->surface.rgb, (size_t)(3 * V + 3)));
    VC_TRY(ensure(ctx, ctx->surface.refined, (size_t)(V + 1)));
    VC_TRY(ensure(ctx, ctx->surface.ctr, 2));
    VC_HIP(ctx, hipMemsetAsync(ctx->surface.ctr.ptr, 0, 2 * sizeof(unsigned long long), ctx->stream));
    if (V) {
        // 2 edge entries in vertex order, the faces (k_mc_faces reads the word bases k_surf_edges writes)
        p.faces = ctx->surface.faces.ptr; p.vcap = V; p.fcap = F;
        const dim3 grid((p.ngroups + 3) / 4), block(kBlock);
        hipLaunchKernelGGL(k_surf_edges, grid, block, 0, ctx->stream, p, ctx->surface.edges.ptr);
        hipLaunchKernelGGL(k_mc_faces, grid, block, 0, ctx->stream, p);
        VC_HIP(ctx, hipGetLastError());
        // 3 the refinement and the colours
        SurfParams q;
        memset(&q, 0, sizeof q);
        q.edges = ctx->surface.edges.ptr;
        q.records = cur.records.ptr;
        q.S = ctx->survivors;
        q.V = V;
        q.xs = ctx->d_axes.ptr; q.ys = q.xs + ctx->nx; q.zs = q.ys + ctx->ny;
        q.bits = s.bits.ptr;
        q.mwords = ctx->mwords; q.C = ctx->C; q.H = ctx->H; q.W = ctx->W;
        q.m = cur.min_views; q.steps = steps; q.order = ctx->surface.order ? 1u : 0u;
        q.nx = ctx->nx; q.ny = ctx->ny;
        q.verts = ctx->surface.verts.ptr; q.rgb = ctx->surface.rgb.ptr; q.refined = ctx->surface.refined.ptr;
        q.ctr = ctx->surface.ctr.ptr;
        memcpy(q.cam, ctx->cams, sizeof(CamDev) * ctx->C);
        hipLaunchKernelGGL(k_surf_refine, dim3((uint32_t)((V + kSurfBlock - 1) / kSurfBlock)), dim3(kSurfBlock), 0, ctx->stream, q);
        VC_HIP(ctx, hipGetLastError());
    }
    VC_TRY(pass_stop(ctx, pass));                   // (the counters' read-back is not part of the mesh's time)
    VC_HIP(ctx, hipMemcpyAsync(ctx->h_res, ctx->surface.ctr.ptr, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VC_TRY(pass_end(ctx, pass, &stats->surface_ms));
    const uint64_t refined = ctx->h_res[0];
    if (refined > V) return fail(ctx, VC_ERR_HIP, "vc_surface_mesh: %llu refined among %llu vertices", (unsigned long long)refined,
                                 (unsigned long long)V);
    ctx->surface.n_verts = V; ctx->surface.n_faces = F; ctx->surface.valid = true; ctx->surface.stamp = ctx->result_gen;
    stats->n_verts = V;
    stats->n_faces = F;
    stats->refined = refined;
    stats->unrefined = V - refined;
    stats->point_tests = ctx->h_res[1];
    return VC_OK;
}

int vc_fetch_surface_mesh(vc_ctx *ctx, double *verts, uint32_t *faces, uint8_t *rgb, uint8_t *refined)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->surface.valid) return fail(ctx, VC_ERR_ARG, "vc_fetch_surface_mesh: no mesh: call vc_surface_mesh first");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t V = (size_t)ctx->surface.n_verts, F = (size_t)ctx->surface.n_faces;
    if (verts && V) VC_HIP(ctx, hipMemcpy(verts, ctx->surface.verts.ptr, V * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (faces && F) VC_HIP(ctx, hipMemcpy(faces, ctx->surface.faces.ptr, F * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (rgb && V) VC_HIP(ctx, hipMemcpy(rgb, ctx->surface.rgb.ptr, V * 3, hipMemcpyDeviceToHost));
    if (refined && V) VC_HIP(ctx, hipMemcpy(refined, ctx->surface.refined.ptr, V, hipMemcpyDeviceToHost));
    return VC_OK;
}
