// ---- geodesic distances through the hull, its extremities and paths (vc_geodesic.h; contract in include/voxcarve.h) ----
// d_geo_acc: [0] the largest d, [1] the reached records, [2] the distinct seeds, [3] the first seed that is no survivor,
// [4, 6) k_geo_source's answer.  d_geo_cnt: [0, 2) the entries of the two tile lists, [2] the picked record, [3] the sweeps' change
// flag, [4, 6) k_geo_path's answer.  h_geo: [0, 8) accumulators, [8] two counters (u32), [10] the word scan's total.
constexpr uint32_t kGeoAccBest = 0, kGeoAccSeeds = 2, kGeoAccBad = 3, kGeoAccOut = 4, kGeoAccTotal = 6;
constexpr uint32_t kGeoCntPick = 2, kGeoCntFlag = 3, kGeoCntPath = 4, kGeoCntTotal = 6;
constexpr uint32_t kGeoSweepsPerRound = 8;
constexpr uint32_t kGeoMaxBlocks = 4096;

// (isqrt(4 s) + 1) div 2: sqrt(s) rounded to the nearest integer (s < 2^42)
static uint64_t geo_edge_um(uint64_t s)
{
    const uint64_t t = 4 * s;
    uint64_t r = (uint64_t)sqrtl((long double)t);
    while (r * r > t) --r;
    while ((r + 1) * (r + 1) <= t) ++r;
    return (r + 1) / 2;
}

// Relaxes from the keys as they are until nothing falls.  Tile route: list 0 holds n0 tiles.  Counts into stats.
static int geo_relax(vc_ctx *ctx, const GeoParams &p, uint32_t connectivity, uint32_t n0, vc_geodesic_stats_t *stats)
{
    uint32_t *hc = reinterpret_cast<uint32_t *>(ctx->geodesic.h + 8);
    const dim3 block(kGeoBlock);
    uint64_t rounds = 0;
    if (ctx->geodesic.tiles) {
        uint32_t par = 0, n = n0;
        while (n) {
            if (++rounds > p.S + 1) return fail(ctx, VC_ERR_INTERNAL, "vc_hull_geodesic: the tiles have not settled after %llu rounds", (unsigned long long)(p.S + 1));
            if (connectivity == 6) VC_DLAUNCH(VC_K_GEO_TILES, k_geo_tiles<6>, dim3(n), block, p, par);
            else if (connectivity == 18) VC_DLAUNCH(VC_K_GEO_TILES, k_geo_tiles<18>, dim3(n), block, p, par);
            else VC_DLAUNCH(VC_K_GEO_TILES, k_geo_tiles<26>, dim3(n), block, p, par);
            VC_HIP(ctx, hipGetLastError());
            VC_HIP(ctx, hipMemcpyAsync(hc, p.count + (par ^ 1u), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VC_HIP(ctx, hipMemsetAsync(p.count + par, 0, sizeof(uint32_t), ctx->stream));
            VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            stats->tile_visits += n;
            stats->launches += 1;
            n = hc[0];
            if ((uint64_t)n > stats->tiles) return fail(ctx, VC_ERR_HIP, "vc_hull_geodesic: %u tiles listed of %llu", n, (unsigned long long)stats->tiles);
            par ^= 1u;
        }
        // (both lists are empty and every flag is clear: the next relaxation starts at parity 0 again)
    } else {
        const dim3 sgrid((uint32_t)((p.S + kGeoBlock - 1) / kGeoBlock));
        uint32_t *flag = ctx->geodesic.cnt.ptr + kGeoCntFlag;
        for (;;) {
            if (++rounds > p.S + 1) return fail(ctx, VC_ERR_INTERNAL, "vc_hull_geodesic: the sweeps have not settled after %llu rounds", (unsigned long long)(p.S + 1));
            VC_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(uint32_t), ctx->stream));
            for (uint32_t k = 0; k < kGeoSweepsPerRound; ++k) {
                if (connectivity == 6) VC_DLAUNCH(VC_K_GEO_SWEEP, k_geo_sweep<6>, sgrid, block, p, flag);
                else if (connectivity == 18) VC_DLAUNCH(VC_K_GEO_SWEEP, k_geo_sweep<18>, sgrid, block, p, flag);
                else VC_DLAUNCH(VC_K_GEO_SWEEP, k_geo_sweep<26>, sgrid, block, p, flag);
            }
            VC_HIP(ctx, hipGetLastError());
            VC_HIP(ctx, hipMemcpyAsync(hc, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            stats->launches += kGeoSweepsPerRound;
            if (!hc[0]) break;
        }
    }
    stats->rounds += (uint32_t)rounds;
    return VC_OK;
}

// Walks the path from `voxel` into `out` (host), growing d_geo_path when the path is longer than nx + ny + nz voxels.
// status = kGeoPath*.
static int geo_walk(vc_ctx *ctx, const GeoParams &p, uint32_t connectivity, uint32_t voxel, std::vector<uint32_t> &out, uint32_t &status)
{
    uint32_t *hc = reinterpret_cast<uint32_t *>(ctx->geodesic.h + 8);
    uint32_t *res = ctx->geodesic.cnt.ptr + kGeoCntPath;
    const uint64_t hops = (uint64_t)p.nx + p.ny + p.nz;
    uint64_t cap = hops < p.S ? hops : p.S;
    for (int attempt = 0; attempt < 2; ++attempt) {
        VC_TRY(ensure(ctx, ctx->geodesic.path, (size_t)(cap ? cap : 1)));
        hipLaunchKernelGGL(k_geo_path, dim3(1), dim3(64), 0, ctx->stream, p, connectivity, voxel, ctx->geodesic.path.ptr, (uint32_t)cap, p.S, res);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(hc, res, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        status = hc[1];
        out.clear();
        if (status != kGeoPathOk) return VC_OK;
        if ((uint64_t)hc[0] <= cap) break;
        if (attempt == 1 || (uint64_t)hc[0] > p.S) return fail(ctx, VC_ERR_HIP, "a path of %u voxels through %llu survivors", hc[0], (unsigned long long)p.S);
        cap = hc[0];
    }
    out.resize(hc[0]);
    if (hc[0]) VC_HIP(ctx, hipMemcpy(out.data(), ctx->geodesic.path.ptr, (size_t)hc[0] * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_hull_geodesic(vc_ctx *ctx, uint32_t connectivity, uint32_t seed_mode, const uint32_t *seeds, uint64_t n_seeds, uint32_t layers,
                     uint32_t K, uint32_t flags, vc_geodesic_stats_t *stats)
{
    if (!ctx) return VC_ERR_ARG;
    if (!stats) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: stats must not be NULL");
    memset(stats, 0, sizeof *stats);
    if (flags & ~VC_GEO_PATHS) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: unknown flags %u (VC_GEO_PATHS)", flags);
    if (connectivity != 6 && connectivity != 18 && connectivity != 26)
        return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: connectivity %u, expected 6, 18 or 26", connectivity);
    Pass pass;
    VC_TRY(pass_open(ctx, "vc_hull_geodesic", "measure", "geodesic distances", pass));
    if (K > VC_GEO_MAX_K) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: K = %u not in [0, %d]", K, VC_GEO_MAX_K);
    if (seed_mode > VC_GEO_SEEDS_IZ_MIN) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: seed mode %u, expected 0 (list), 1 (iz max) or 2 (iz min)", seed_mode);
    if (seed_mode == VC_GEO_SEEDS_LIST && n_seeds && !seeds) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: %llu seeds and no list", (unsigned long long)n_seeds);
    if (seed_mode != VC_GEO_SEEDS_LIST && layers < 1) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: layers = 0, a layer mode seeds at least one");
    uint64_t q[3];
    VC_TRY(dist_metric(ctx, "vc_hull_geodesic", q));
    const uint64_t S = pass.S, n = pass.n, nwords = pass.nwords;
    if (n > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: %llu voxels exceed the u32 index", (unsigned long long)n);
    if (seed_mode != VC_GEO_SEEDS_LIST) n_seeds = 0;
    if (!S && n_seeds) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: seed 0 (voxel %u) is no survivor", seeds[0]);
    StepBuf &cur = *pass.cur;
    VC_TRY(pass_begin(ctx));
    ctx->geodesic.stamp = kNever;
    ctx->geodesic.ext.clear();
    ctx->geodesic.paths.clear();
    VC_HIP(ctx, ensure_pinned(ctx->geodesic.h, 12));
    uint64_t *h = ctx->geodesic.h;
    uint32_t *hc = reinterpret_cast<uint32_t *>(h + 8);
    memset(h, 0, 12 * sizeof(uint64_t));
    stats->survivors = S;
    for (int a = 0; a < 3; ++a) stats->q[a] = q[a];
    GeoParams p;
    memset(&p, 0, sizeof p);
    for (uint32_t m = 1; m < 8; ++m) {
        const uint64_t s2 = (m & 1 ? q[0] * q[0] : 0) + (m & 2 ? q[1] * q[1] : 0) + (m & 4 ? q[2] * q[2] : 0);
        stats->edge_um[m - 1] = geo_edge_um(s2);
        p.w8[m] = (unsigned long long)stats->edge_um[m - 1] << 8;
    }
    VC_TRY(pass_start(ctx, pass));
    if (S) {
        // survivors before each word, as vc_hull_components counts them
        VC_TRY(ensure(ctx, ctx->d_rscan, word_groups(nwords)));
        VC_TRY(ensure(ctx, ctx->geodesic.woff, (size_t)nwords));
        VC_TRY(word_offsets(ctx, cur, nwords, ctx->geodesic.woff, h + 10));      // (the total is not read; h_res holds the box next)
        // the survivors' box: the tiles are laid from its low corner, the layer modes seed from its iz range
        uint32_t *hb = nullptr;
        VC_TRY(dist_survivor_box(ctx, cur, S, hb));
        uint64_t tiles = 1;
        const uint32_t tdim[3] = {kGeoTX, kGeoTY, kGeoTZ};
        for (int a = 0; a < 3; ++a) {
            p.lo[a] = hb[a];
            p.nt[a] = (hb[3 + a] - hb[a]) / tdim[a] + 1;
            tiles *= p.nt[a];
        }
        const uint32_t zlo = hb[2], zhi = hb[5];
        stats->tiles = tiles;
        if (tiles > 0xffffffffull) return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: %llu tiles exceed the u32 index", (unsigned long long)tiles);
        p.tiles = (uint32_t)tiles;
        VC_TRY(ensure(ctx, ctx->geodesic.key, (size_t)S));
        VC_TRY(ensure(ctx, ctx->geodesic.acc, kGeoAccTotal));
        VC_TRY(ensure(ctx, ctx->geodesic.cnt, kGeoCntTotal));
        VC_TRY(ensure(ctx, ctx->geodesic.flag, (size_t)(2 * tiles)));
        VC_TRY(ensure(ctx, ctx->geodesic.list, (size_t)(2 * tiles)));
        if (n_seeds) VC_TRY(ensure(ctx, ctx->geodesic.seeds, (size_t)n_seeds));
        p.records = cur.records.ptr; p.words = cur.words.ptr; p.woff = ctx->geodesic.woff.ptr; p.key = ctx->geodesic.key.ptr;
        p.S = S; p.nx = ctx->nx; p.ny = ctx->ny; p.nz = ctx->nz;
        p.flag[0] = ctx->geodesic.flag.ptr; p.flag[1] = ctx->geodesic.flag.ptr + tiles;
        p.list[0] = ctx->geodesic.list.ptr; p.list[1] = ctx->geodesic.list.ptr + tiles;
        p.count = ctx->geodesic.cnt.ptr;
        unsigned long long *acc = ctx->geodesic.acc.ptr;
        uint32_t *pick = ctx->geodesic.cnt.ptr + kGeoCntPick;
        VC_HIP(ctx, hipMemsetAsync(p.key, 0xff, (size_t)S * sizeof(uint64_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(ctx->geodesic.flag.ptr, 0, (size_t)(2 * tiles) * sizeof(uint32_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(ctx->geodesic.cnt.ptr, 0, kGeoCntTotal * sizeof(uint32_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(acc, 0, kGeoAccTotal * sizeof(uint64_t), ctx->stream));
        VC_HIP(ctx, hipMemsetAsync(acc + kGeoAccBad, 0xff, sizeof(uint64_t), ctx->stream));
        const dim3 block(kGeoBlock);
        // item 2: the seed set
        if (seed_mode == VC_GEO_SEEDS_LIST) {
            if (n_seeds) {
                VC_HIP(ctx, hipMemcpyAsync(ctx->geodesic.seeds.ptr, seeds, (size_t)n_seeds * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
                VC_DLAUNCH(VC_K_GEO_SEED, k_geo_seed_list, dim3((uint32_t)((n_seeds + kGeoBlock - 1) / kGeoBlock)), block, p,
                           (const uint32_t *)ctx->geodesic.seeds.ptr, n_seeds, n, acc + kGeoAccSeeds);
            }
        } else {
            const uint32_t span = layers - 1 < zhi - zlo ? layers - 1 : zhi - zlo;
            const uint32_t z0 = seed_mode == VC_GEO_SEEDS_IZ_MAX ? zhi - span : zlo, z1 = seed_mode == VC_GEO_SEEDS_IZ_MAX ? zhi : zlo + span;
            VC_DLAUNCH(VC_K_GEO_SEED, k_geo_seed_layers, dim3((uint32_t)((S + kGeoBlock - 1) / kGeoBlock)), block, p, z0, z1, acc + kGeoAccSeeds);
        }
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(h + kGeoAccSeeds, acc + kGeoAccSeeds, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipMemcpyAsync(hc, p.count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h[kGeoAccBad] != ~0ull) {
            dist_harvest(ctx);
            const uint64_t bad = h[kGeoAccBad];
            return fail(ctx, VC_ERR_ARG, "vc_hull_geodesic: seed %llu (voxel %u) is no survivor", (unsigned long long)bad, bad < n_seeds ? seeds[bad] : 0u);
        }
        stats->seeds = h[kGeoAccSeeds];
        if (stats->seeds > S || (uint64_t)hc[0] > tiles)
            return fail(ctx, VC_ERR_HIP, "vc_hull_geodesic: %llu seeds in %u tiles of %llu survivors", (unsigned long long)stats->seeds, hc[0], (unsigned long long)S);
        VC_TRY(geo_relax(ctx, p, connectivity, hc[0], stats));
        // item 3: farthest point, two passes; the path back before the point becomes a source
        const uint64_t gblocks = (S + kGeoBlock - 1) / kGeoBlock;
        const dim3 ggrid((uint32_t)(gblocks < kGeoMaxBlocks ? gblocks : kGeoMaxBlocks));
        for (uint32_t k = 1; k <= K && stats->seeds; ++k) {
            VC_HIP(ctx, hipMemsetAsync(acc + kGeoAccBest, 0, 2 * sizeof(uint64_t), ctx->stream));
            VC_HIP(ctx, hipMemsetAsync(pick, 0xff, sizeof(uint32_t), ctx->stream));
            VC_DLAUNCH(VC_K_GEO_ARGMAX, k_geo_best, ggrid, block, (const unsigned long long *)p.key, S, acc + kGeoAccBest);
            VC_DLAUNCH(VC_K_GEO_ARGMAX, k_geo_pick, ggrid, block, (const unsigned long long *)p.key, S, (const unsigned long long *)(acc + kGeoAccBest), pick);
            VC_HIP(ctx, hipGetLastError());
            std::vector<uint32_t> way;
            if (flags & VC_GEO_PATHS) {
                VC_HIP(ctx, hipMemcpyAsync(h + kGeoAccBest, acc + kGeoAccBest, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
                VC_HIP(ctx, hipMemcpyAsync(hc, pick, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
                VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
                if (h[kGeoAccBest] == 0 || (uint64_t)hc[0] >= S) break;
                uint64_t rec = 0;
                VC_HIP(ctx, hipMemcpy(&rec, cur.records.ptr + hc[0], sizeof rec, hipMemcpyDeviceToHost));
                uint32_t status = kGeoPathOk;
                VC_TRY(geo_walk(ctx, p, connectivity, (uint32_t)rec, way, status));
                if (status != kGeoPathOk) return fail(ctx, VC_ERR_HIP, "vc_hull_geodesic: the path of extremity %u ended with status %u", k, status);
            }
            VC_DLAUNCH(VC_K_GEO_SEED, k_geo_source, dim3(1), dim3(64), p, (const unsigned long long *)(acc + kGeoAccBest), (const uint32_t *)pick, k,
                       acc + kGeoAccOut);
            VC_HIP(ctx, hipGetLastError());
            VC_HIP(ctx, hipMemcpyAsync(h + kGeoAccOut, acc + kGeoAccOut, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
            VC_HIP(ctx, hipMemcpyAsync(hc, p.count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const uint64_t d = h[kGeoAccOut];
            const uint32_t rec = (uint32_t)h[kGeoAccOut + 1], voxel = (uint32_t)(h[kGeoAccOut + 1] >> 32);
            if (d == 0 || rec == 0xffffffffu) break;
            vc_extremum_t e;
            memset(&e, 0, sizeof e);
            e.d = d; e.voxel = voxel; e.record = rec; e.label = k;
            e.iy = voxel % ctx->ny; e.ix = (voxel / ctx->ny) % ctx->nx; e.iz = voxel / (ctx->ny * ctx->nx);
            ctx->geodesic.ext.push_back(e);
            if (flags & VC_GEO_PATHS) ctx->geodesic.paths.push_back(std::move(way));
            VC_TRY(geo_relax(ctx, p, connectivity, hc[0], stats));
        }
        VC_HIP(ctx, hipMemsetAsync(acc + kGeoAccBest, 0, 2 * sizeof(uint64_t), ctx->stream));
        VC_DLAUNCH(VC_K_GEO_ARGMAX, k_geo_best, ggrid, block, (const unsigned long long *)p.key, S, acc + kGeoAccBest);
        VC_HIP(ctx, hipGetLastError());
        VC_HIP(ctx, hipMemcpyAsync(h + kGeoAccBest, acc + kGeoAccBest, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    VC_TRY(pass_end(ctx, pass, &stats->geodesic_ms));
    if (h[kGeoAccBest + 1] > S) return fail(ctx, VC_ERR_HIP, "vc_hull_geodesic: %llu reached of %llu survivors", (unsigned long long)h[kGeoAccBest + 1], (unsigned long long)S);
    stats->max_d = S ? h[kGeoAccBest] : 0;
    stats->reached = S ? h[kGeoAccBest + 1] : 0;
    stats->unreached = S - stats->reached;
    stats->extremities = (uint32_t)ctx->geodesic.ext.size();
    ctx->geodesic.p = p;
    ctx->geodesic.stamp = ctx->result_gen;
    ctx->geodesic.n = S; ctx->geodesic.max_d = stats->max_d; ctx->geodesic.conn = connectivity;
    return VC_OK;
}

// The refusal the readers of the geodesic outputs share.
static int geodesic_current(vc_ctx *ctx)
{
    if (!ctx->carved || !ctx->current(ctx->geodesic.stamp)) return fail(ctx, VC_ERR_ARG, "no geodesic distances: call vc_hull_geodesic on the current carve result");
    return VC_OK;
}

// The keys of the last call, on the host.
static int geo_fetch_keys(vc_ctx *ctx, std::vector<uint64_t> &keys)
{
    VC_HIP(ctx, hipSetDevice(ctx->device));
    keys.resize((size_t)ctx->geodesic.n);
    if (ctx->geodesic.n) VC_HIP(ctx, hipMemcpy(keys.data(), ctx->geodesic.key.ptr, (size_t)ctx->geodesic.n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return VC_OK;
}

int vc_fetch_geodesic(vc_ctx *ctx, uint64_t *d)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(geodesic_current(ctx));
    if (!d) return VC_OK;                        // only asked whether the distances are valid
    std::vector<uint64_t> keys;
    VC_TRY(geo_fetch_keys(ctx, keys));
    for (size_t s = 0; s < keys.size(); ++s) d[s] = keys[s] == kGeoNone ? kGeoNone : keys[s] >> 8;
    return VC_OK;
}

int vc_fetch_geodesic_labels(vc_ctx *ctx, uint8_t *labels)
{
    if (!ctx || !labels) return VC_ERR_ARG;
    VC_TRY(geodesic_current(ctx));
    std::vector<uint64_t> keys;
    VC_TRY(geo_fetch_keys(ctx, keys));
    for (size_t s = 0; s < keys.size(); ++s) labels[s] = (uint8_t)(keys[s] & 255u);     // (2^64 - 1 gives 255)
    return VC_OK;
}

int vc_fetch_extrema(vc_ctx *ctx, vc_extremum_t *out)
{
    if (!ctx) return VC_ERR_ARG;
    VC_TRY(geodesic_current(ctx));
    if (!ctx->geodesic.ext.empty()) {
        if (!out) return VC_ERR_ARG;
        memcpy(out, ctx->geodesic.ext.data(), ctx->geodesic.ext.size() * sizeof(vc_extremum_t));
    }
    return VC_OK;
}

// *n = the path's length; out takes it when capacity holds it.
static int geo_path_out(vc_ctx *ctx, const char *what, const std::vector<uint32_t> &way, uint32_t *out, uint32_t capacity, uint32_t *n)
{
    *n = (uint32_t)way.size();
    if (way.size() > capacity) return fail(ctx, VC_ERR_ARG, "%s: the path has %zu voxels, the capacity is %u", what, way.size(), capacity);
    if (!way.empty()) {
        if (!out) return VC_ERR_ARG;
        memcpy(out, way.data(), way.size() * sizeof(uint32_t));
    }
    return VC_OK;
}

int vc_geodesic_path(vc_ctx *ctx, uint32_t voxel, uint32_t *out, uint32_t capacity, uint32_t *n)
{
    if (!ctx || !n) return VC_ERR_ARG;
    *n = 0;
    VC_TRY(geodesic_current(ctx));
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if ((uint64_t)voxel >= ctx->n_voxels() || !ctx->geodesic.n) return fail(ctx, VC_ERR_ARG, "vc_geodesic_path: voxel %u is no survivor", voxel);
    VC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> way;
    uint32_t status = kGeoPathOk;
    VC_TRY(geo_walk(ctx, ctx->geodesic.p, ctx->geodesic.conn, voxel, way, status));
    if (status == kGeoPathNoSurvivor) return fail(ctx, VC_ERR_ARG, "vc_geodesic_path: voxel %u is no survivor", voxel);
    if (status == kGeoPathUnreached) return fail(ctx, VC_ERR_ARG, "vc_geodesic_path: voxel %u is unreached", voxel);
    if (status != kGeoPathOk) return fail(ctx, VC_ERR_HIP, "vc_geodesic_path: the walk from voxel %u found no next voxel", voxel);
    return geo_path_out(ctx, "vc_geodesic_path", way, out, capacity, n);
}

int vc_fetch_extremum_path(vc_ctx *ctx, uint32_t k, uint32_t *out, uint32_t capacity, uint32_t *n)
{
    if (!ctx || !n) return VC_ERR_ARG;
    *n = 0;
    VC_TRY(geodesic_current(ctx));
    if (ctx->geodesic.paths.size() != ctx->geodesic.ext.size() || (ctx->geodesic.ext.size() && ctx->geodesic.paths.empty()))
        return fail(ctx, VC_ERR_ARG, "vc_fetch_extremum_path: vc_hull_geodesic ran without VC_GEO_PATHS");
    if (k < 1 || k > ctx->geodesic.paths.size()) return fail(ctx, VC_ERR_ARG, "vc_fetch_extremum_path: k = %u not in [1, %zu]", k, ctx->geodesic.paths.size());
    return geo_path_out(ctx, "vc_fetch_extremum_path", ctx->geodesic.paths[k - 1], out, capacity, n);
}

int vc_paint_geodesic(vc_ctx *ctx, uint32_t mode, const uint8_t *palette)
{
    if (!ctx) return VC_ERR_ARG;
    if (mode > VC_GEO_PAINT_DISTANCE) return fail(ctx, VC_ERR_ARG, "vc_paint_geodesic: mode %u, expected 0 (labels) or 1 (distance)", mode);
    if (mode == VC_GEO_PAINT_LABELS && !palette) return fail(ctx, VC_ERR_ARG, "vc_paint_geodesic: no palette");
    VC_TRY(geodesic_current(ctx));
    if (ctx->npending) return fail(ctx, VC_ERR_ARG, "carve steps are in flight: collect them with vc_carve_end first");
    if (!ctx->geodesic.n) return VC_OK;
    StepBuf &cur = ctx->sb[ctx->cur];
    VC_HIP(ctx, hipSetDevice(ctx->device));
    GeoPalette pal;
    memset(&pal, 0, sizeof pal);
    if (palette)
        for (uint32_t k = 0; k <= kGeoMaxK; ++k) pal.rgb[k] = (uint32_t)palette[3 * k] | ((uint32_t)palette[3 * k + 1] << 8) | ((uint32_t)palette[3 * k + 2] << 16);
    const uint32_t none = (uint32_t)VC_GEO_UNREACHED_R | ((uint32_t)VC_GEO_UNREACHED_G << 8) | ((uint32_t)VC_GEO_UNREACHED_B << 16);
    hipLaunchKernelGGL(k_geo_paint, dim3((uint32_t)((ctx->geodesic.n + kGeoBlock - 1) / kGeoBlock)), dim3(kGeoBlock), 0, ctx->stream, cur.records.ptr,
                       ctx->geodesic.n, (const unsigned long long *)ctx->geodesic.key.ptr, mode, (unsigned long long)ctx->geodesic.max_d, none, pal);
    VC_HIP(ctx, hipGetLastError());
    VC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return VC_OK;
}
