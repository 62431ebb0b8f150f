/* rt_light_table.h — the light table of include/rt_nee.h (amendment 1), built on the host from the caller's arrays; plain C++, no HIP, so
 * that a host test reaches it (tests/light_table_driver.cpp) and rt_debug_light_table needs no device.  The header text there defines
 * every bit of the table; this file follows it line by line.  The double arithmetic must not be contracted (-ffp-contract=off, as every
 * host file of the library is built). */
#ifndef RT_LIGHT_TABLE_H
#define RT_LIGHT_TABLE_H

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/rt_nee.h"

namespace rt_lt {

struct LightTable {
    std::vector<RtLightEntry> entries;
    std::vector<float> cdf;
    std::vector<uint32_t> inTable; /* per object (spheres, then models): 1 = the object has an entry (amendment 3) */
    int nSphere = 0, nTriangle = 0;
    bool empty() const { return entries.empty(); }
};

/* Le and whether the material makes its object an emitter */
inline bool emitter(const RtMaterial& m, float le[3])
{
    bool finite = true, positive = false;
    for (int k = 0; k < 3; k++) {
        le[k] = m.emissionCol[k] * m.emissionStrength;
        finite = finite && std::isfinite(le[k]);
        positive = positive || le[k] > 0.0f;
    }
    return m.flag != RT_MATERIAL_GLASS && finite && positive;
}

inline float max3(const float v[3]) { return std::max(v[0], std::max(v[1], v[2])); }

/* mul(localToWorld, float4(p, 1)).xyz, summed left to right (rt_math.h, rt_mul_point) */
inline void to_world(const float* m, const float* p, float out[3])
{
    for (int r = 0; r < 3; r++) out[r] = m[r] * p[0] + m[4 + r] * p[1] + m[8 + r] * p[2] + m[12 + r] * 1.0f;
}

inline double linear_det(const float* m)
{
    const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10]; /* rows (a b c), (d e f), (g h i) */
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}

/* end of a model's triangle range: the smallest triOffset above its own, or nTris */
inline void triangle_ends(const RtModel* models, int nModels, int nTris, std::vector<int>& end)
{
    std::vector<int> offs(nModels);
    for (int i = 0; i < nModels; i++) offs[i] = models[i].triOffset;
    std::sort(offs.begin(), offs.end());
    end.assign(nModels, nTris);
    for (int i = 0; i < nModels; i++) {
        auto it = std::upper_bound(offs.begin(), offs.end(), models[i].triOffset);
        if (it != offs.end()) end[i] = *it;
    }
}

/* The table of a scene.  `corners`: the local-space corners of triangle t are the nine floats at corners + t * strideFloats (an
 * RtTriangle array: stride 18).  RT_OK, RT_ERR_INVALID_ARG (*why) or RT_ERR_SCENE (the cap; *why). */
inline int build(const RtModel* models, int nModels, const float* corners, size_t strideFloats, int nTris, const RtSphere* spheres, int nSpheres, LightTable& t,
                 const char** why, long long maxLights = RT_NEE_MAX_LIGHTS)
{
    *why = "";
    t = LightTable();
    if (nModels < 0 || nTris < 0 || nSpheres < 0 || (nModels && !models) || (nTris && !corners) || (nSpheres && !spheres)) {
        *why = "bad pointer/count";
        return RT_ERR_INVALID_ARG;
    }
    for (int i = 0; i < nModels; i++)
        if (models[i].triOffset < 0 || models[i].triOffset > nTris) {
            *why = "a model's triOffset is outside [0, n_triangles]";
            return RT_ERR_INVALID_ARG;
        }
    t.inTable.assign((size_t)nSpheres + nModels, 0u);
    std::vector<double> weight;
    for (int s = 0; s < nSpheres; s++) {
        float le[3];
        const float r = spheres[s].radius;
        if (!emitter(spheres[s].material, le) || !(r > 0.0f) || !std::isfinite(r)) continue;
        if ((long long)t.entries.size() >= maxLights) { *why = "more emitters than RT_NEE_MAX_LIGHTS"; return RT_ERR_SCENE; }
        RtLightEntry e;
        memset(&e, 0, sizeof(e));
        memcpy(e.a, spheres[s].centre, 12);
        e.size = r * r;
        e.object = s;
        e.triangle = -1;
        memcpy(e.emission, le, 12);
        t.entries.push_back(e);
        weight.push_back((4.0 * M_PI * ((double)r * (double)r)) * (double)max3(le));
        t.inTable[s] = 1u;
        t.nSphere++;
    }
    std::vector<int> end;
    triangle_ends(models, nModels, nTris, end);
    {   /* one allocation for the entries a scene of emissive meshes will make (at most the cap + 1: the build stops there) */
        long long want = (long long)t.entries.size();
        for (int m = 0; m < nModels && want <= maxLights; m++) {
            float le[3];
            if (emitter(models[m].material, le)) want += end[m] - models[m].triOffset;
        }
        t.entries.reserve((size_t)(want < maxLights ? want : maxLights));
        weight.reserve(t.entries.capacity());
    }
    for (int m = 0; m < nModels; m++) {
        float le[3];
        if (!emitter(models[m].material, le)) continue;
        const float* l2w = models[m].localToWorld;
        const bool mirrored = linear_det(l2w) < 0.0;
        for (int k = models[m].triOffset; k < end[m]; k++) {
            const float* p = corners + (size_t)k * strideFloats;
            float A[3], B[3], C[3];
            to_world(l2w, p, A);
            to_world(l2w, p + (mirrored ? 6 : 3), B);
            to_world(l2w, p + (mirrored ? 3 : 6), C);
            RtLightEntry e;
            memset(&e, 0, sizeof(e));
            double E1[3], E2[3];
            for (int d = 0; d < 3; d++) {
                e.a[d] = A[d];
                e.e1[d] = B[d] - A[d];
                e.e2[d] = C[d] - A[d];
                E1[d] = (double)B[d] - (double)A[d];
                E2[d] = (double)C[d] - (double)A[d];
            }
            const double X[3] = {E1[1] * E2[2] - E1[2] * E2[1], E1[2] * E2[0] - E1[0] * E2[2], E1[0] * E2[1] - E1[1] * E2[0]};
            const double L = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
            const float S = (float)(0.5 * L);
            for (int d = 0; d < 3; d++) e.ng[d] = (float)(X[d] / L);
            if (!(S > 0.0f) || !std::isfinite(S) || !std::isfinite(e.ng[0]) || !std::isfinite(e.ng[1]) || !std::isfinite(e.ng[2])) continue;
            if ((long long)t.entries.size() >= maxLights) { *why = "more emitters than RT_NEE_MAX_LIGHTS"; return RT_ERR_SCENE; }
            e.size = S;
            e.object = nSpheres + m;
            e.triangle = k;
            memcpy(e.emission, le, 12);
            t.entries.push_back(e);
            weight.push_back((double)S * (double)max3(le));
            t.inTable[(size_t)nSpheres + m] = 1u;
            t.nTriangle++;
        }
    }
    const size_t n = t.entries.size();
    double total = 0.0;
    for (size_t i = 0; i < n; i++) total += weight[i];
    t.cdf.resize(n);
    double run = 0.0;
    for (size_t i = 0; i < n; i++) {
        run += weight[i];
        t.cdf[i] = (float)(run / total);
        t.entries[i].prob = (float)(weight[i] / total);
    }
    if (n) t.cdf[n - 1] = 1.0f;
    return RT_OK;
}

/* The reverse map of include/rt_mis.h: from a hit (object, triangle) to the index of its entry in `t`, NO_ENTRY (0xffffffff) where it
 * has none.  objects: one word per object — a sphere's entry, or the index into `triangles` of the word of a model's first triangle.
 * triangles: for every model with an entry, one word per triangle of its range [triOffset, end), in model order; triCount[o] is that
 * range's length (0 for a sphere or a model without an entry).  `t` must be build()'s table of the same arrays. */
struct LightMap {
    enum : uint32_t { NO_ENTRY = 0xffffffffu };
    std::vector<uint32_t> objects, triOffset, triCount, triangles;
};

inline void build_map(const LightTable& t, const RtModel* models, int nModels, int nTris, int nSpheres, LightMap& map)
{
    const size_t nObjects = (size_t)nSpheres + (size_t)nModels;
    map.objects.assign(nObjects, (uint32_t)LightMap::NO_ENTRY);
    map.triOffset.assign(nObjects, 0u);
    map.triCount.assign(nObjects, 0u);
    map.triangles.clear();
    std::vector<int> end;
    triangle_ends(models, nModels, nTris, end);
    size_t words = 0;
    for (int m = 0; m < nModels; m++) {
        const size_t o = (size_t)nSpheres + m;
        if (o >= t.inTable.size() || !t.inTable[o]) continue;
        map.objects[o] = (uint32_t)words;
        map.triOffset[o] = (uint32_t)models[m].triOffset;
        map.triCount[o] = (uint32_t)(end[m] - models[m].triOffset);
        words += map.triCount[o];
    }
    map.triangles.assign(words, (uint32_t)LightMap::NO_ENTRY);
    for (size_t i = 0; i < t.entries.size(); i++) {
        const RtLightEntry& e = t.entries[i];
        if (e.object < 0 || (size_t)e.object >= nObjects) continue;
        if (e.triangle < 0) {
            map.objects[e.object] = (uint32_t)i;
            continue;
        }
        const uint32_t rel = (uint32_t)e.triangle - map.triOffset[e.object];
        if (map.objects[e.object] != LightMap::NO_ENTRY && rel < map.triCount[e.object]) map.triangles[(size_t)map.objects[e.object] + rel] = (uint32_t)i;
    }
}

/* rt_debug_light_table / rt_debug_light_table_free without the error text */
inline int dump(const RtModel* models, int nModels, const RtTriangle* triangles, int nTris, const RtSphere* spheres, int nSpheres, RtLightTableDump* out, const char** why)
{
    *why = "";
    if (!out) { *why = "null output"; return RT_ERR_INVALID_ARG; }
    memset(out, 0, sizeof(*out));
    LightTable t;
    try {
        const int rc = build(models, nModels, reinterpret_cast<const float*>(triangles), sizeof(RtTriangle) / sizeof(float), nTris, spheres, nSpheres, t, why);
        if (rc) return rc;
    } catch (const std::bad_alloc&) {
        *why = "out of host memory";
        return RT_ERR_OOM;
    }
    const size_t n = t.entries.size();
    out->entries = (RtLightEntry*)malloc(n ? n * sizeof(RtLightEntry) : 1);
    out->cdf = (float*)malloc(n ? n * sizeof(float) : 1);
    if (!out->entries || !out->cdf) {
        free(out->entries);
        free(out->cdf);
        memset(out, 0, sizeof(*out));
        *why = "out of host memory";
        return RT_ERR_OOM;
    }
    if (n) {
        memcpy(out->entries, t.entries.data(), n * sizeof(RtLightEntry));
        memcpy(out->cdf, t.cdf.data(), n * sizeof(float));
    }
    out->n_entries = (int32_t)n;
    out->n_sphere_entries = t.nSphere;
    out->n_triangle_entries = t.nTriangle;
    return RT_OK;
}

inline void dump_free(RtLightTableDump* d)
{
    if (!d) return;
    free(d->entries);
    free(d->cdf);
    memset(d, 0, sizeof(*d));
}

} // namespace rt_lt

#endif /* RT_LIGHT_TABLE_H */
