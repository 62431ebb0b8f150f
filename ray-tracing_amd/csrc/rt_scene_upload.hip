/*
 * rt_scene_upload.hip — the device half of the scene upload: what rt_scene_prep.h prepared goes to the context's device
 * (commit_scene, also rt_multi.hip's), and the per-frame update calls refresh what moved, stream-ordered.  No kernel is launched here.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <new>
#include <vector>

#include "rt_context.h"
#include "rt_scene_prep.h"

void free_scene(RtContext* ctx)
{
    hipFree(ctx->dSpheres); ctx->dSpheres = nullptr;
    hipFree(ctx->dMaterials); ctx->dMaterials = nullptr;
    hipFree(ctx->dModels); ctx->dModels = nullptr;
    hipFree(ctx->dPairs); ctx->dPairs = nullptr;
    hipFree(ctx->dTris); ctx->dTris = nullptr;
    hipFree(ctx->dNorms); ctx->dNorms = nullptr;
    hipFree(ctx->dUnitTri); ctx->dUnitTri = nullptr;
    hipFree(ctx->dBigLeaves); ctx->dBigLeaves = nullptr;
    hipFree(ctx->dFilters); ctx->dFilters = nullptr;
    hipFree(ctx->dChunks); ctx->dChunks = nullptr;
    ctx->nChunks = 0;
    ctx->haveScene = false;
}

/* ---------------------------------------------------------------- scene */

template <typename T>
static int upload_vec(RtContext* ctx, T** dptr, const void* src, size_t count)
{
    size_t bytes = count * sizeof(T);
    HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : sizeof(T)));
    if (bytes) HIP_TRY(ctx, hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

/* the filter boxes moved: the chunk boxes (and the spatial clustering) follow, stream-ordered */
static int refresh_chunks(RtContext* ctx, const std::vector<DFilter>& filters)
{
    if (!ctx->nChunks) return RT_OK;
    std::vector<DChunk> chunks;
    int nf = 0, ew = 0;
    make_chunks(filters, chunks, &nf, &ew);
    if ((int)chunks.size() != ctx->nChunks) { /* a model became (un)filterable: the split into chunks changed size — rare, synchronous */
        HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
        hipFree(ctx->dChunks);
        ctx->dChunks = nullptr;
        int rc = upload_vec(ctx, &ctx->dChunks, chunks.data(), chunks.size());
        if (rc) return rc;
        ctx->nChunks = (int)chunks.size();
        return RT_OK;
    }
    return stage_upload(ctx, ctx->dChunks, chunks.data(), sizeof(DChunk) * chunks.size());
}

/* the models' matrices or the spheres (the scene extent) moved: the root filter boxes again, from the context's root records, then the chunks */
static int refresh_filters(RtContext* ctx, const RtModel* models, const std::vector<RtSphere>& spheres)
{
    std::vector<DFilter> filters;
    make_filters(models, ctx->nModels, ctx->hRootCodes, ctx->hRootChildren, spheres.data(), (int)spheres.size(), filters, &ctx->filterMaxOrigin);
    {
        const std::vector<DFilter> up = append_filter_pairs(filters);
        if (int rc = stage_upload(ctx, ctx->dFilters, up.data(), sizeof(DFilter) * up.size())) return rc;
    }
    return refresh_chunks(ctx, filters);
}


/* device copy of one scene array: from the host vector, or — `peer` — from the context that already holds it, device to
 * device on this context's stream (xGMI when the devices differ; the caller synchronises the stream) */
template <typename T, typename V>
static int commit_vec(RtContext* ctx, T** dptr, const V& v, T* const* peerPtr, const RtContext* peer)
{
    if (!peer) return upload_vec(ctx, dptr, v.data(), v.size());
    const size_t bytes = v.size() * sizeof(T);
    HIP_TRY(ctx, hipMalloc(dptr, bytes ? bytes : sizeof(T)));
    if (bytes) HIP_TRY(ctx, hipMemcpyPeerAsync(*dptr, ctx->device, *peerPtr, peer->device, bytes, ctx->stream));
    return RT_OK;
}

int commit_scene(RtContext* ctx, const PreparedScene& ps, const RtContext* peer)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(joined(ctx)));
    free_scene(ctx);
    int rc;
    if ((rc = commit_vec(ctx, &ctx->dSpheres, ps.sph, peer ? &peer->dSpheres : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dMaterials, ps.mats, peer ? &peer->dMaterials : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dModels, ps.dmodels, peer ? &peer->dModels : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dPairs, ps.lay.pairBuf, peer ? &peer->dPairs : nullptr, peer))) return rc;
    if (!ps.lay.arena && (rc = commit_vec(ctx, &ctx->dTris, ps.lay.triBuf, peer ? &peer->dTris : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dNorms, ps.lay.normBuf, peer ? &peer->dNorms : nullptr, peer))) return rc;
    if (ps.lay.unitTri.size() && (rc = commit_vec(ctx, &ctx->dUnitTri, ps.lay.unitTri, peer ? &peer->dUnitTri : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dBigLeaves, ps.lay.bigLeaves, peer ? &peer->dBigLeaves : nullptr, peer))) return rc;
    ctx->arenaLayout = ps.lay.arena;
    ctx->layoutUsed = ps.lay.used.name();
    if ((rc = commit_vec(ctx, &ctx->dFilters, ps.filters, peer ? &peer->dFilters : nullptr, peer))) return rc;
    if ((rc = commit_vec(ctx, &ctx->dChunks, ps.chunks, peer ? &peer->dChunks : nullptr, peer))) return rc;
    ctx->nChunks = (int)ps.chunks.size();
    ctx->nFiltered = ps.nFiltered;
    ctx->extWords = ps.extWords;
    ctx->filterMaxOrigin = ps.maxOrigin;
    ctx->sphereBound = ps.sphereBound;
    ctx->hRootChildren = ps.rootChildren;
    ctx->hSpheres = ps.hSpheres;
    ctx->nSpheres = (int)ps.hSpheres.size();
    ctx->nModels = (int)ps.hModels.size();
    ctx->nTris = ps.nTris;
    ctx->nPairs = (int)ps.nPairs;
    ctx->hTriBase = ps.lay.triBase;
    {
        const auto& triSpace = ps.lay.arena ? ps.lay.pairBuf : ps.lay.triBuf;
        primary_collect_tris(ps.flat, ps.dmodels.data(), (int)ps.dmodels.size(), triSpace.data(), triSpace.size(), ps.lay.bigLeaves.data(), ps.lay.bigLeaves.size(), ctx->primaryTris);
    }
    ctx->stackEntries = ps.flat ? 0 : ps.maxHeight; /* (the FLAT variant pushes nothing: its LDS is pixel bookkeeping only) */
    ctx->flatScene = ps.flat;
    ctx->hotUnits = ps.flat ? 0u : ps.lay.hotUnits;
    {   /* one ray, one segment: every model once (a step each), every pair and every leaf of its tree at most once — and the same tree once
         * per model that uses it.  64 lanes, one step of one lane per iteration at least; the factor 2 is slack, not arithmetic. */
        const unsigned long long steps = (unsigned long long)ps.hModels.size() * (2ull * ps.nPairs + 2ull) + 16ull;
        const unsigned long long lim = 2ull * 64ull * steps;
        ctx->travLimit = lim > 0x7fffffffull ? 0x7fffffffu : (uint32_t)lim;
        if (const char* e = getenv("RT_TRAV_LIMIT")) ctx->travLimit = (uint32_t)strtoul(e, nullptr, 10); /* test hook: make the watchdog fire */
    }
    ctx->wavesPerGroup = ctx->hotUnits ? ps.wavesPerGroup : 1;
    {   /* the FLAT variant's chain pool (rt_kernels.h, pool_exchange): 16-wave workgroups (two per CU at the variant's 8 waves per SIMD), two
         * queues of 64 cells of 128 bytes — 17 KB of the workgroup's 70 KB.  RT_POOL=0: single-wave workgroups without a pool (rounds 1-5);
         * RT_POOL_WAVES: A/B runs and tests */
        int on = 1, waves = RT_MAX_WAVES_PER_GROUP_FLAT;
        if (const char* e = getenv("RT_POOL")) on = atoi(e);
        if (const char* e = getenv("RT_POOL_WAVES")) waves = atoi(e);
        if (waves < 1) waves = 1;
        if (waves > RT_MAX_WAVES_PER_GROUP_FLAT) waves = RT_MAX_WAVES_PER_GROUP_FLAT;
        const bool pooled = ps.flat && on;
        ctx->poolWaves = pooled ? waves : 1;
        ctx->poolCells = pooled ? (int)RT_POOL_CELLS : 0;
    }
    ctx->hModels = ps.hModels;
    ctx->hRootCodes = ps.rootCodes;
    try {
        ctx->hCorners.resize((size_t)ps.nTris * 9); /* (ps.srcTris: the caller's array, alive for the upload call this runs in) */
    } catch (const std::bad_alloc&) {
        return fail(ctx, RT_ERR_OOM, "rt_upload_scene: out of host memory keeping the triangles' corners");
    }
    for (size_t k = 0; k < (size_t)ps.nTris; k++) memcpy(&ctx->hCorners[9 * k], ps.srcTris[k].posA, 36);
    ctx->lightDirty = true;
    ctx->haveScene = true;
    ctx->tuner.done = getenv("RT_SUSPEND") != nullptr; /* RT_SUSPEND=3|4 pins the threshold (tests, A/B runs) */
    ctx->tuner.decided = ctx->tuner.done ? atoi(getenv("RT_SUSPEND")) : 3;
    if (ctx->tuner.decided < 1 || ctx->tuner.decided > 7) ctx->tuner.decided = 3;
    ctx->tuner.ms[0] = ctx->tuner.ms[1] = 0;
    ctx->tuner.n[0] = ctx->tuner.n[1] = 0;
    ctx->tuner.next = 0;
    for (auto& pr : ctx->tuner.probe) pr.live = false;
    return RT_OK;
}

extern "C" {

int rt_upload_scene(RtContext* ctx, const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                    const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    RT_FLUSH(ctx);
    PreparedScene ps;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, spheres, n_spheres, ps);
    if (rc) return fail(ctx, rc, "%s", ps.error.c_str());
    const auto t1 = std::chrono::steady_clock::now();
    rc = commit_scene(ctx, ps, nullptr);
    if (getenv("RT_DEBUG_UPLOAD"))
        fprintf(stderr, "[rt] rt_upload_scene: prepare %.2f ms, commit %.2f ms (%d triangles, %zu node pairs)\n",
                std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(), n_triangles, ps.nPairs);
    return rc;
}

int rt_validate_scene(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                      const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres, RtSceneInfo* out_info)
{
    PreparedScene ps;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, spheres, n_spheres, ps);
    if (rc) fail(nullptr, rc, "%s", ps.error.c_str());
    if (out_info) {
        memset(out_info, 0, sizeof(*out_info));
        out_info->prepare_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc == RT_OK) {
            out_info->n_pairs = (int32_t)ps.nPairs;
            out_info->max_height = ps.maxHeight;
            out_info->flat = ps.flat ? 1 : 0;
            out_info->n_filtered = ps.nFiltered;
        }
    }
    return rc;
}

int rt_debug_layout(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                    const RtBVHNode* nodes, int n_nodes, const char* layout, RtLayoutDump* out)
{
    if (!out) return fail(nullptr, RT_ERR_INVALID_ARG, "rt_debug_layout: null output");
    memset(out, 0, sizeof(*out));
    PreparedScene ps;
    const int rc = prepare_scene(models, n_models, triangles, n_triangles, nodes, n_nodes, nullptr, 0, ps, layout);
    if (rc) return fail(nullptr, rc, "%s", ps.error.c_str());
    auto take = [](PodVec<unsigned char>& v, unsigned char** p, size_t* n) { *p = v.p; *n = v.n; v.p = nullptr; v.n = 0; };
    take(ps.lay.pairBuf, &out->pair_space, &out->pair_bytes);
    take(ps.lay.triBuf, &out->tri_space, &out->tri_bytes);
    take(ps.lay.normBuf, &out->norm_space, &out->norm_bytes);
    auto dup = [](const void* src, size_t bytes) { void* q = malloc(bytes ? bytes : 1); if (q && bytes) memcpy(q, src, bytes); return q; };
    out->n_big_leaves = ps.lay.bigLeaves.size() / 2;
    out->big_leaves = (uint32_t*)dup(ps.lay.bigLeaves.data(), ps.lay.bigLeaves.size() * 4);
    out->root_codes = (uint32_t*)dup(ps.lay.rootCodes.data(), ps.lay.rootCodes.size() * 4);
    out->tri_base = (int32_t*)dup(ps.lay.triBase.data(), ps.lay.triBase.size() * 4);
    out->n_models = n_models;
    out->arena = ps.lay.arena ? 1 : 0;
    snprintf(out->used, sizeof(out->used), "%s", ps.lay.used.name().c_str());
    return RT_OK;
}

void rt_debug_layout_free(RtLayoutDump* d)
{
    if (!d) return;
    free(d->pair_space); free(d->tri_space); free(d->norm_space); free(d->big_leaves); free(d->root_codes); free(d->tri_base);
    memset(d, 0, sizeof(*d));
}

int rt_update_models(RtContext* ctx, const RtModel* models, int n_models)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "rt_update_models before rt_upload_scene");
    if (n_models != ctx->nModels || (n_models && !models)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_update_models: model count changed (%d != %d)", n_models, ctx->nModels);
    if (n_models == 0) return RT_OK;
    /* RCM:192-204 runs every frame; in a static scene nothing changed: no device work at all */
    if (memcmp(models, ctx->hModels.data(), sizeof(RtModel) * (size_t)n_models) == 0) {
        ctx->updateSkips++;
        return RT_OK;
    }
    RT_FLUSH(ctx); /* frames held back were requested with the old models */
    std::vector<DModel> dmodels(n_models);
    std::vector<DMaterial> mats(n_models);
    bool matricesChanged = false;
    for (int i = 0; i < n_models; i++) {
        if (models[i].nodeOffset != ctx->hModels[i].nodeOffset || models[i].triOffset != ctx->hModels[i].triOffset)
            return fail(ctx, RT_ERR_INVALID_ARG, "rt_update_models: model %d changed its BVH offsets; re-upload the scene", i);
        pack_model(models[i], ctx->hRootCodes[i], ctx->hTriBase[i], dmodels[i]);
        pack_material(models[i].material, mats[i]);
        if (memcmp(models[i].worldToLocal, ctx->hModels[i].worldToLocal, sizeof(models[i].worldToLocal)) != 0 ||
            memcmp(models[i].localToWorld, ctx->hModels[i].localToWorld, sizeof(models[i].localToWorld)) != 0)
            matricesChanged = true;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* stream-ordered: lands after the frames already enqueued, before the next launch */
    int rc;
    /* (a failure from here on may leave device memory ahead of the host mirrors the table of origin constants is built from:
     * the table then stays off until the next rt_upload_scene — rt_primary.h) */
    if ((rc = stage_upload(ctx, ctx->dModels, dmodels.data(), sizeof(DModel) * n_models))) { ctx->primaryTris.usable = false; return rc; }
    if ((rc = stage_upload(ctx, ctx->dMaterials + ctx->nSpheres, mats.data(), sizeof(DMaterial) * n_models))) { ctx->primaryTris.usable = false; return rc; }
    if (matricesChanged) { /* the world-space root filter boxes depend on the matrices only */
        if ((rc = refresh_filters(ctx, models, ctx->hSpheres))) { ctx->primaryTris.usable = false; return rc; }
    }
    ctx->hModels.assign(models, models + n_models);
    ctx->lightDirty = true;
    return RT_OK;
}

int rt_update_spheres(RtContext* ctx, const RtSphere* spheres, int n_spheres)
{
    if (!ctx) return fail(nullptr, RT_ERR_INVALID_ARG, "null context");
    if (!ctx->haveScene) return fail(ctx, RT_ERR_STATE, "rt_update_spheres before rt_upload_scene");
    if (n_spheres != ctx->nSpheres || (n_spheres && !spheres)) return fail(ctx, RT_ERR_INVALID_ARG, "rt_update_spheres: sphere count changed");
    if (n_spheres == 0) return RT_OK;
    if (memcmp(spheres, ctx->hSpheres.data(), sizeof(RtSphere) * (size_t)n_spheres) == 0) {
        ctx->updateSkips++;
        return RT_OK;
    }
    RT_FLUSH(ctx);
    std::vector<float> sph;
    float bound = 0.0f;
    pack_spheres(spheres, n_spheres, sph, &bound);
    std::vector<DMaterial> mats(n_spheres);
    for (int i = 0; i < n_spheres; i++) pack_material(spheres[i].material, mats[i]);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    /* (the bound and the mirror change together with the device records; a failure after the first upload leaves the table of origin
     * constants off until the next rt_upload_scene, as in rt_update_models) */
    if ((rc = stage_upload(ctx, ctx->dSpheres, sph.data(), sph.size() * 4))) { ctx->primaryTris.usable = false; return rc; }
    ctx->sphereBound = bound;
    if ((rc = stage_upload(ctx, ctx->dMaterials, mats.data(), sizeof(DMaterial) * n_spheres))) { ctx->primaryTris.usable = false; return rc; }
    ctx->hSpheres.assign(spheres, spheres + n_spheres);
    ctx->lightDirty = true;
    if (ctx->nModels) { /* the filter margins scale with the scene extent, which includes the spheres */
        if ((rc = refresh_filters(ctx, ctx->hModels.data(), ctx->hSpheres))) return rc;
    }
    return RT_OK;
}

} /* extern "C" */
