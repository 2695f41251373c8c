// ---- marching cubes over the dense ON/OFF volume (reference consumer voxel_reconstruction.py:127-163) ----
int vc_marching_cubes(vc_ctx *ctx, const uint8_t *volume_bits, uint32_t d0, uint32_t d1, uint32_t d2, float level,
                      uint64_t *n_verts, uint64_t *n_faces)
{
    if (!ctx || !n_verts || !n_faces) return VC_ERR_ARG;
    *n_verts = *n_faces = 0;
    ctx->mc_valid = false;
    if (d0 == 0 || d1 == 0 || d2 == 0) return fail(ctx, VC_ERR_ARG, "volume dimensions must be >= 1");
    if (!(level >= 0.0f && level < 1.0f)) return fail(ctx, VC_ERR_ARG, "level %g not in [0, 1): ON is 1, OFF is 0", (double)level);
    const uint64_t n = (uint64_t)d0 * d1 * d2;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "volume of %llu elements exceeds the u32 index", (unsigned long long)n);
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t nwords = (uint32_t)((n + 63) / 64), ngroups = (nwords + 63) / 64;
    const uint32_t nscan = (ngroups + kScanBlock - 1) / kScanBlock;
    McParams p;
    memset(&p, 0, sizeof p);
    if (volume_bits) {
        VC_TRY(ensure(ctx, ctx->d_mcbits, (size_t)nwords));
        VC_HIP(ctx, hipMemsetAsync(ctx->d_mcbits.ptr, 0, (size_t)nwords * sizeof(uint64_t), ctx->stream));
        VC_HIP(ctx, hipMemcpyAsync(ctx->d_mcbits.ptr, volume_bits, (size_t)((n + 7) / 8), hipMemcpyHostToDevice, ctx->stream));
        p.bits = ctx->d_mcbits.ptr;
    } else {
        if (!ctx->carved) return fail(ctx, VC_ERR_ARG, "no carve result: run vc_carve first or pass a volume");
        if (n != ctx->n_voxels()) return fail(ctx, VC_ERR_ARG, "%u x %u x %u is not the %llu voxels of the carved slab", d0, d1, d2,
                                              (unsigned long long)ctx->n_voxels());
        StepBuf &cur = ctx->sb[ctx->cur];
        VC_TRY(densify_words(ctx, cur));
        p.bits = cur.words.ptr;
    }
    VC_TRY(ensure(ctx, ctx->d_mcx, (size_t)nwords * 3));
    VC_TRY(ensure(ctx, ctx->d_mcwbase, (size_t)nwords));
    VC_TRY(ensure(ctx, ctx->d_mcv, ngroups));
    VC_TRY(ensure(ctx, ctx->d_mct, ngroups));
    VC_TRY(ensure_exchange_scratch(ctx, 1));
    p.n = n; p.d0 = d0; p.d1 = d1; p.d2 = d2; p.nwords = nwords; p.ngroups = ngroups;
    p.x = ctx->d_mcx.ptr; p.wbase = ctx->d_mcwbase.ptr; p.gv = ctx->d_mcv.cnt.ptr; p.gt = ctx->d_mct.cnt.ptr;
    p.gvoff = ctx->d_mcv.off.ptr; p.gtoff = ctx->d_mct.off.ptr; p.bvoff = ctx->d_mcv.boff.ptr; p.btoff = ctx->d_mct.boff.ptr;
    p.level = level;
    const dim3 grid((ngroups + 3) / 4), block(kBlock);
    hipLaunchKernelGGL(k_mc_count, grid, block, 0, ctx->stream, p);
    VC_HIP(ctx, hipGetLastError());
    VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_mcv, ctx->d_mcv.cnt.ptr, ngroups, ctx->h_xtotal));
    VC_TRY(scan_counts(ctx, ctx->stream, ctx->d_mct, ctx->d_mct.cnt.ptr, ngroups, ctx->h_xtotal + 1));
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)nscan;
    const uint64_t V = ctx->h_xtotal[0], F = ctx->h_xtotal[1];
    if (V > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "%llu vertices exceed the u32 vertex number", (unsigned long long)V);
    VC_TRY(ensure(ctx, ctx->d_mcverts, (size_t)(3 * V + 3)));
    VC_TRY(ensure(ctx, ctx->d_mcfaces, (size_t)(3 * F + 3)));
    p.verts = ctx->d_mcverts.ptr; p.faces = ctx->d_mcfaces.ptr; p.vcap = V; p.fcap = F;
    hipLaunchKernelGGL(k_mc_verts, grid, block, 0, ctx->stream, p);
    hipLaunchKernelGGL(k_mc_faces, grid, block, 0, ctx->stream, p);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mc_verts = V; ctx->mc_faces = F; ctx->mc_valid = true;
    *n_verts = V; *n_faces = F;
    return VC_OK;
}

int vc_fetch_mesh(vc_ctx *ctx, float *verts, uint32_t *faces)
{
    if (!ctx) return VC_ERR_ARG;
    if (!ctx->mc_valid) return fail(ctx, VC_ERR_ARG, "no mesh: call vc_marching_cubes");
    VC_HIP(ctx, hipSetDevice(ctx->device));
    if (verts && ctx->mc_verts) VC_HIP(ctx, hipMemcpy(verts, ctx->d_mcverts.ptr, ctx->mc_verts * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (faces && ctx->mc_faces) VC_HIP(ctx, hipMemcpy(faces, ctx->d_mcfaces.ptr, ctx->mc_faces * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VC_OK;
}
