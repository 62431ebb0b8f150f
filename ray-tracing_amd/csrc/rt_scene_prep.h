/*
 * rt_scene_prep.h — the host half of rt_upload_scene (internal; plain C++, no HIP): the caller's arrays are validated and re-laid
 * out ONCE into what the kernels read (rt_records.h), ready to be uploaded to any number of contexts.
 *
 * The arrays are UNTRUSTED: SceneBuilder::convert follows the caller's node indices, and every index is checked before it is
 * used.  The root filter boxes (make_filters) and the chunk hierarchy (make_chunks) are conservative stand-ins for whole models:
 * a box that is too small does not crash, it drops geometry.  tests/scene_prep_driver.cpp compiles this header into a
 * stand-alone program (tests/test_scene_prep.py runs it under the address and undefined-behaviour sanitizers).
 * rt_scene_upload.hip holds the device half (commit_scene, refresh_filters) and reports prepare_scene's message on its context.
 */
#ifndef RT_SCENE_PREP_H
#define RT_SCENE_PREP_H

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/rt_abi.h"
#include "rt_records.h"
#include "rt_layout.h"
#include "rt_launch_plan.h"

/* Device sphere records.  First the exact one the reference's arithmetic reads — centre and
 * radius*radius (RC:299, same fp32 multiply) — then, for all spheres again, the record of the
 * conservative discriminant pre-test in begin_intersect: centre and |c|^2 - r*r (rounded from
 * double).  *bound = max_k(|c_k|^2 + r_k^2), rounded up: it scales the pre-test's error margin. */
static inline void pack_spheres(const RtSphere* spheres, int n, std::vector<float>& out, float* bound)
{
    /* n exact records (c, r*r), then ceil(n/2) PAIR records of the conservative pre-test: (cx0, cx1, cy0, cy1, cz0, cz1, K0, K1)
     * with K = |c|^2 - r*r — two spheres side by side, so that one scalar load fills the SGPR pairs a packed fp32
     * instruction takes (begin_intersect); an odd last sphere is paired with itself */
    const size_t pairs = ((size_t)n + 1) / 2;
    out.assign((size_t)n * 4 + pairs * 8, 0.0f);
    double maxM = 0;
    for (int i = 0; i < n; i++) {
        const float* c = spheres[i].centre;
        const float r2 = spheres[i].radius * spheres[i].radius;
        memcpy(&out[4 * (size_t)i], c, 12);
        out[4 * (size_t)i + 3] = r2;
        const double cc = (double)c[0] * c[0] + (double)c[1] * c[1] + (double)c[2] * c[2];
        const float K = (float)(cc - (double)r2);
        float* q = &out[4 * (size_t)n + 8 * (size_t)(i / 2)];
        const int h = i & 1;
        q[0 + h] = c[0]; q[2 + h] = c[1]; q[4 + h] = c[2]; q[6 + h] = K;
        if (!h && i == n - 1) { q[1] = c[0]; q[3] = c[1]; q[5] = c[2]; q[7] = K; }
        if (cc + (double)r2 > maxM) maxM = cc + (double)r2;
    }
    *bound = (float)(maxM * 1.000001);
}

static inline void pack_material(const RtMaterial& m, DMaterial& d)
{
    memset(&d, 0, sizeof(d));
    memcpy(d.diffuseCol, m.diffuseCol, 16);
    memcpy(d.emissionCol, m.emissionCol, 16);
    memcpy(d.specularCol, m.specularCol, 16);
    memcpy(d.absorption, m.absorption, 16);
    d.absorptionStrength = m.absorptionStrength;
    d.emissionStrength = m.emissionStrength;
    d.smoothness = m.smoothness;
    d.specularProbability = m.specularProbability;
    d.ior = m.ior;
    d.flag = m.flag;
}
static inline void pack_model(const RtModel& m, uint32_t rootCode, int32_t triBaseUnits, DModel& d)
{
    memset(&d, 0, sizeof(d));
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            d.w2l[r * 4 + c] = m.worldToLocal[c * 4 + r];
            d.l2w[r * 4 + c] = m.localToWorld[c * 4 + r];
        }
    d.rootCode = rootCode;
    d.triBase = triBaseUnits;
    d.cullBackface = m.material.flag != RT_MATERIAL_GLASS; /* RC:355 */
}

/* World-space, inflated boxes of a model's two root children — the conservative root filter
 * of begin_intersect.  Corners go through inverse(worldToLocal) in double precision; the
 * inflation (1e-4 of the scene extent plus 1e-5 of the model's own coordinate range, mapped to
 * world units) is two to three orders of magnitude above the fp32 rounding of the reference's
 * local-space slab test.  A matrix that is not affine-invertible in a well-conditioned way
 * disables the filter for that model. */
static inline bool invert_affine(const float* m /* column-major 4x4 */, double inv[12] /* 3 rows x 4 */)
{
    double a[3][3], t[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) a[r][c] = m[c * 4 + r];
        t[r] = m[12 + r];
    }
    if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f) return false;
    double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                 a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    double scale = 0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) scale = fmax(scale, fabs(a[r][c]));
    if (!(fabs(det) > 1e-9 * scale * scale * scale) || !std::isfinite(det)) return false;
    double id = 1.0 / det;
    double b[3][3];
    b[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) * id; b[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * id; b[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * id;
    b[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) * id; b[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * id; b[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * id;
    b[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) * id; b[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * id; b[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * id;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) inv[r * 4 + c] = b[r][c];
        inv[r * 4 + 3] = -(b[r][0] * t[0] + b[r][1] * t[1] + b[r][2] * t[2]);
        for (int c = 0; c < 4; c++)
            if (!std::isfinite(inv[r * 4 + c])) return false;
    }
    return true;
}

/* returns false if the model cannot be filtered; otherwise world boxes (not yet inflated) in wmin/wmax[2][3] */
static inline bool world_boxes(const RtModel& m, const RtBVHNode children[2], double wmin[2][3], double wmax[2][3], double* localRange)
{
    double inv[12];
    if (!invert_affine(m.worldToLocal, inv)) return false;
    double range = 0, normS = 0;
    for (int r = 0; r < 3; r++) normS = fmax(normS, fabs(inv[r * 4]) + fabs(inv[r * 4 + 1]) + fabs(inv[r * 4 + 2]));
    for (int k = 0; k < 2; k++) {
        for (int d = 0; d < 3; d++) {
            if (!std::isfinite(children[k].boundsMin[d]) || !std::isfinite(children[k].boundsMax[d])) return false;
            wmin[k][d] = INFINITY;
            wmax[k][d] = -INFINITY;
            range = fmax(range, fmax(fabs((double)children[k].boundsMin[d]), fabs((double)children[k].boundsMax[d])));
        }
        for (int corner = 0; corner < 8; corner++) {
            double p[3];
            for (int d = 0; d < 3; d++) p[d] = (corner >> d & 1) ? children[k].boundsMax[d] : children[k].boundsMin[d];
            for (int r = 0; r < 3; r++) {
                double w = inv[r * 4] * p[0] + inv[r * 4 + 1] * p[1] + inv[r * 4 + 2] * p[2] + inv[r * 4 + 3];
                wmin[k][r] = fmin(wmin[k][r], w);
                wmax[k][r] = fmax(wmax[k][r], w);
            }
        }
    }
    *localRange = range * normS;
    return true;
}

static inline void make_filters(const RtModel* models, int n_models, const std::vector<uint32_t>& rootCodes, const std::vector<RtBVHNode>& rootChildren,
                                const RtSphere* spheres, int n_spheres, std::vector<DFilter>& out, float* maxOrigin)
{
    out.assign(n_models, DFilter());
    std::vector<double> lr(n_models, 0.0);
    std::vector<char> ok(n_models, 0);
    std::vector<double> bmin((size_t)n_models * 6), bmax((size_t)n_models * 6);
    double extent = 0;
    for (int i = 0; i < n_models; i++) {
        DFilter& f = out[i];
        memset(&f, 0, sizeof(f));
        /* innerRoot: bit 0 = the root is an inner node; a leaf root carries its triangle count in bits 8.. (exact
         * counters of rejected models).  rootChildren holds the root's two child boxes, or — leaf root — the
         * bounds of the leaf's triangles twice (computed from the triangles on upload, never taken from the
         * root node, whose bounds the reference does not read) */
        const bool leafRoot = (rootCodes[i] & RT_CODE_LEAF) != 0;
        f.innerRoot = leafRoot ? ((uint32_t)rootChildren[2 * (size_t)i].triangleCount << 8) : 1u;
        f.always = 1;
        if (leafRoot && rootChildren[2 * (size_t)i].triangleCount <= 0) continue; /* no box available */
        double wmin[2][3], wmax[2][3];
        if (!world_boxes(models[i], &rootChildren[2 * (size_t)i], wmin, wmax, &lr[i])) continue;
        ok[i] = 1;
        for (int k = 0; k < 2; k++)
            for (int d = 0; d < 3; d++) {
                bmin[(size_t)i * 6 + k * 3 + d] = wmin[k][d];
                bmax[(size_t)i * 6 + k * 3 + d] = wmax[k][d];
                extent = fmax(extent, fmax(fabs(wmin[k][d]), fabs(wmax[k][d])));
            }
    }
    for (int i = 0; i < n_spheres; i++)
        for (int d = 0; d < 3; d++) extent = fmax(extent, fabs((double)spheres[i].centre[d]) + fabs((double)spheres[i].radius));
    if (!std::isfinite(extent)) extent = 0;
    for (int i = 0; i < n_models; i++) {
        if (!ok[i]) continue;
        DFilter& f = out[i];
        const double margin = 1e-4 * extent + 1e-5 * lr[i] + 1e-30;
        bool fin = true;
        for (int d = 0; d < 3; d++) { /* one box: the union of the two children (measured cheaper than testing both) */
            const double lo2 = fmin(bmin[(size_t)i * 6 + d], bmin[(size_t)i * 6 + 3 + d]);
            const double hi2 = fmax(bmax[(size_t)i * 6 + d], bmax[(size_t)i * 6 + 3 + d]);
            float lo = nextafterf((float)(lo2 - margin), -INFINITY);
            float hi = nextafterf((float)(hi2 + margin), INFINITY);
            f.bMin[d] = lo;
            f.bMax[d] = hi;
            fin = fin && std::isfinite(lo) && std::isfinite(hi);
        }
        f.always = fin ? 0u : 1u;
    }
    /* rays starting farther than this from the origin have coarser fp32 spacing than the margin allows for */
    *maxOrigin = (float)(8.0 * extent);
}

/* The device array behind KArgs::filters / filterPairs: the n DFilter records, then ceil(n / 2) pair records (two DFilter
 * slots each) with the same boxes side by side for the packed root filter of rt_kernels.h. */
static inline std::vector<DFilter> append_filter_pairs(const std::vector<DFilter>& f)
{
    const size_t n = f.size(), np = (n + 1) / 2;
    std::vector<DFilter> out(n + 2 * np);
    if (!out.empty()) memset(out.data(), 0, out.size() * sizeof(DFilter)); /* (no models: data() may be null, which memset must not be given) */
    for (size_t i = 0; i < n; i++) out[i] = f[i];
    static_assert(sizeof(DFilter) == 32, "a pair record is two DFilter slots = sixteen dwords");
    for (size_t p = 0; p < np; p++) {
        float* q = reinterpret_cast<float*>(&out[n + 2 * p]);
        for (int h = 0; h < 2; h++) {
            const size_t m = 2 * p + h;
            uint32_t always = 1u; /* a missing second model never reaches the mask (the kernel checks m + 1 < n) */
            if (m < n) {
                for (int d = 0; d < 3; d++) {
                    q[2 * d + h] = f[m].bMin[d];
                    q[6 + 2 * d + h] = f[m].bMax[d];
                }
                always = f[m].always;
            }
            memcpy(&q[12 + h], &always, 4);
        }
    }
    return out;
}

/* Chunks of the two-level model hierarchy (rt_records.h, DChunk): only built for more than 64 models.
 * Models the filter cannot reject (`always`) are kept in chunks of their own so that they do not spoil the
 * boxes of the others; the rest is clustered by the Morton code of the filter box centre. */
static inline void make_chunks(const std::vector<DFilter>& filters, std::vector<DChunk>& chunks, int* nFiltered, int* extWords)
{
    const int n = (int)filters.size();
    chunks.clear();
    const rt_plan::Filtering fl = rt_plan::filtering(n);
    *nFiltered = fl.nFiltered;
    *extWords = fl.extWords;
    if (n <= 64) return;
    const int nf = fl.nFiltered;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int i = 0; i < nf; i++)
        if (!filters[i].always)
            for (int d = 0; d < 3; d++) {
                lo[d] = fmin(lo[d], (double)filters[i].bMin[d]);
                hi[d] = fmax(hi[d], (double)filters[i].bMax[d]);
            }
    auto spread = [](uint32_t v) { /* 10 bits -> every third bit */
        v &= 1023u;
        v = (v | (v << 16)) & 0x030000ffu;
        v = (v | (v << 8)) & 0x0300f00fu;
        v = (v | (v << 4)) & 0x030c30c3u;
        v = (v | (v << 2)) & 0x09249249u;
        return v;
    };
    std::vector<std::pair<uint64_t, int>> order;
    for (int i = 0; i < nf; i++) {
        uint64_t key;
        if (filters[i].always) {
            key = (uint64_t)i; /* first, in index order */
        } else {
            uint32_t q[3];
            for (int d = 0; d < 3; d++) {
                const double c = 0.5 * ((double)filters[i].bMin[d] + (double)filters[i].bMax[d]);
                const double t = hi[d] > lo[d] ? (c - lo[d]) / (hi[d] - lo[d]) : 0.0;
                q[d] = (uint32_t)(t < 0 ? 0 : t > 1 ? 1023 : t * 1023.0);
            }
            key = (1ull << 40) | ((uint64_t)(spread(q[0]) | (spread(q[1]) << 1) | (spread(q[2]) << 2)) << 8);
        }
        order.push_back({key, i});
    }
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, int>& a, const std::pair<uint64_t, int>& b) { return a.first < b.first; });
    for (size_t p = 0; p < order.size();) {
        DChunk c;
        memset(&c, 0, sizeof(c));
        const bool alw = filters[order[p].second].always != 0;
        c.always = alw ? 1u : 0u;
        for (int d = 0; d < 3; d++) { c.bMin[d] = INFINITY; c.bMax[d] = -INFINITY; }
        while (p < order.size() && c.count < RT_CHUNK_MODELS && (filters[order[p].second].always != 0) == alw) {
            const DFilter& f = filters[order[p].second];
            c.members[c.count++] = (uint32_t)order[p].second;
            c.innerRoots += f.innerRoot & 1u;
            if (!alw)
                for (int d = 0; d < 3; d++) {
                    c.bMin[d] = fminf(c.bMin[d], f.bMin[d]);
                    c.bMax[d] = fmaxf(c.bMax[d], f.bMax[d]);
                }
            p++;
        }
        std::sort(c.members, c.members + c.count);
        chunks.push_back(c);
    }
}

struct SceneBuilder {
    const RtBVHNode* nodes;
    int nNodes, nTris;
    std::vector<DPair> pairs;
    std::vector<uint32_t> bigLeaves;
    std::vector<int32_t> pairOfFirstChild; /* absolute first-child node index -> pair id, -1 unseen, -2 in progress */
    std::vector<int32_t> pairDepth;        /* height of the subtree below pair (levels) */
    std::vector<int32_t> pairNodeOffset;   /* the nodeOffset the pair's inner children were resolved with (RC:265-266: child = nodeOffset + startIndex) */
    std::vector<long long> pairLeafEnd;    /* largest startIndex + triangleCount of the leaves below pair (mesh-relative) */
    std::string error;
    /* parallel conversion (one builder per mesh): pairs go into a segment of the scene's array, with their final ids; the memo
     * covers only the mesh's own node window.  A mesh that leaves its window or overflows its segment sets `outside` and the
     * caller falls back to the sequential walk, which has neither limit. */
    DPair* seg = nullptr;
    size_t segCap = 0, segCount = 0;
    uint32_t idBase = 0;
    int memoLo = 0;
    bool outside = false;

    /* code of a leaf node whose triangles are [start, start+count) relative to triOffset */
    bool leaf_code(const RtBVHNode& n, int triOffset, uint32_t* code)
    {
        long long lo = (long long)triOffset + n.startIndex, hi = lo + n.triangleCount;
        if (n.startIndex < 0 || lo < 0 || hi > nTris) {
            error = "leaf triangle range out of bounds";
            return false;
        }
        if (n.triangleCount <= RT_CODE_MAX_INLINE_COUNT && (uint32_t)n.startIndex <= RT_CODE_MAX_INLINE_START) {
            *code = RT_CODE_LEAF | ((uint32_t)n.triangleCount << 24) | (uint32_t)n.startIndex;
        } else {
            uint32_t idx = (uint32_t)(bigLeaves.size() / 2);
            if (idx > RT_CODE_MAX_INLINE_START) { error = "too many oversized leaves"; return false; }
            bigLeaves.push_back((uint32_t)n.startIndex);
            bigLeaves.push_back((uint32_t)n.triangleCount);
            *code = RT_CODE_LEAF | idx;
        }
        return true;
    }

    /* Converts the subtree under node `abs` (absolute index) of a mesh whose node 0 is at nodeOffset.
     * Returns its code and height (leaf = 0). Iterative post-order walk, memoised per sibling pair. */
    bool convert(int nodeOffset, int triOffset, int absRoot, uint32_t* codeOut, int* heightOut, long long* endOut = nullptr)
    {
        struct Frame { int abs; int stage; int firstChild; uint32_t codeA, codeB; int hA, hB; long long endA; };
        std::vector<Frame> stack;
        stack.push_back({absRoot, 0, -1, 0, 0, 0, 0, 0});
        uint32_t retCode = 0;
        int retHeight = 0;
        long long retEnd = 0; /* largest leaf end (mesh-relative) of the subtree just returned */
        while (!stack.empty()) {
            Frame& f = stack.back();
            const RtBVHNode& n = nodes[f.abs];
            if (f.stage == 0) {
                if (n.triangleCount > 0) { /* leaf — RC:246 */
                    if (!leaf_code(n, triOffset, &retCode)) return false;
                    retHeight = 0;
                    retEnd = (long long)n.startIndex + n.triangleCount;
                    stack.pop_back();
                    continue;
                }
                long long fc = (long long)nodeOffset + n.startIndex;
                if (n.startIndex < 0 || fc < 0 || fc + 1 >= nNodes) { error = "inner node child index out of bounds"; return false; }
                f.firstChild = (int)fc;
                if (f.firstChild < memoLo || (size_t)(f.firstChild - memoLo) >= pairOfFirstChild.size()) { outside = true; error = "node outside the mesh's window"; return false; }
                int known = pairOfFirstChild[f.firstChild - memoLo];
                if (known == -2) { error = "cycle in BVH node graph"; return false; }
                if (known >= 0) {
                    /* a pair with inner children means what it means under ONE nodeOffset (RC:265-266 adds the model's nodeOffset to a child
                     * index): a mesh whose tree wanders into another mesh's nodes would need a second, different conversion of the same nodes —
                     * refused like a cycle (the reference would traverse it; no builder produces it) */
                    if (pairDepth[known - idBase] > 1 && pairNodeOffset[known - idBase] != nodeOffset) { error = "node pair reached under two different nodeOffsets"; return false; }
                    /* converted for an earlier model that shares these nodes: its leaves were range-checked
                     * against THAT model's triOffset, so check this one's against the subtree's largest leaf end */
                    if ((long long)triOffset + pairLeafEnd[known - idBase] > nTris) { error = "leaf triangle range out of bounds"; return false; }
                    retCode = (uint32_t)known;
                    retHeight = pairDepth[known - idBase];
                    retEnd = pairLeafEnd[known - idBase];
                    stack.pop_back();
                    continue;
                }
                if ((int)stack.size() > RT_MAX_BVH_DEPTH + 1) { error = "BVH deeper than RT_MAX_BVH_DEPTH"; return false; }
                pairOfFirstChild[f.firstChild - memoLo] = -2;
                f.stage = 1;
                int child = f.firstChild;
                stack.push_back({child, 0, -1, 0, 0, 0, 0, 0});
                continue;
            }
            if (f.stage == 1) {
                f.codeA = retCode;
                f.hA = retHeight;
                f.endA = retEnd;
                f.stage = 2;
                int child = f.firstChild + 1;
                stack.push_back({child, 0, -1, 0, 0, 0, 0, 0});
                continue;
            }
            /* stage 2: both children done */
            f.codeB = retCode;
            f.hB = retHeight;
            const RtBVHNode& A = nodes[f.firstChild];
            const RtBVHNode& B = nodes[f.firstChild + 1];
            DPair p;
            memset(&p, 0, sizeof(p));
            memcpy(p.aMin, A.boundsMin, 12); memcpy(p.aMax, A.boundsMax, 12);
            memcpy(p.bMin, B.boundsMin, 12); memcpy(p.bMax, B.boundsMax, 12);
            p.codeA = f.codeA;
            p.codeB = f.codeB;
            int id;
            if (seg) {
                if (segCount == segCap) { outside = true; error = "more node pairs than the mesh's window holds"; return false; }
                seg[segCount] = p;
                id = (int)(idBase + segCount++);
            } else {
                id = (int)pairs.size();
                pairs.push_back(p);
            }
            int h = 1 + (f.hA > f.hB ? f.hA : f.hB);
            pairDepth.push_back(h);
            pairNodeOffset.push_back(nodeOffset);
            pairLeafEnd.push_back(f.endA > retEnd ? f.endA : retEnd);
            pairOfFirstChild[f.firstChild - memoLo] = id;
            retCode = (uint32_t)id;
            retHeight = h;
            retEnd = pairLeafEnd.back();
            stack.pop_back();
        }
        *codeOut = retCode;
        *heightOut = retHeight;
        if (endOut) *endOut = retEnd;
        return true;
    }
};

/* host worker threads for the scene preparation: f(k) for k in [0, n), at most RT_HOST_THREADS (default 16) at a time */
template <typename F>
static inline void parallel_jobs(int n, F f)
{
    int nThreads = (int)std::thread::hardware_concurrency();
    if (const char* e = getenv("RT_HOST_THREADS")) nThreads = atoi(e);
    if (nThreads > 16) nThreads = 16;
    if (nThreads > n) nThreads = n;
    if (nThreads <= 1) {
        for (int k = 0; k < n; k++) f(k);
        return;
    }
    std::atomic<int> next(0);
    std::vector<std::thread> pool;
    for (int t = 0; t < nThreads; t++)
        pool.emplace_back([&] { for (int k = next.fetch_add(1); k < n; k = next.fetch_add(1)) f(k); });
    for (auto& th : pool) th.join();
}

/* The host side of rt_upload_scene: everything validated and re-laid out ONCE, ready to be uploaded to any number of
 * contexts (rt_multi_upload_scene prepares once for all its devices). */
struct PreparedScene {
    std::vector<float> sph;
    float sphereBound = 0;
    std::vector<DMaterial> mats;
    std::vector<DModel> dmodels;
    PodVec<DPair> pairs; /* canonical form (SceneBuilder::convert); consumed by the layout */
    LaidOutScene lay;    /* what is uploaded: pair / triangle / normal spaces, final codes */
    size_t nPairs = 0;
    std::vector<DFilter> filters;
    std::vector<DChunk> chunks;
    int nFiltered = 0, extWords = 0;
    float maxOrigin = 0;
    std::vector<RtBVHNode> rootChildren;
    std::vector<uint32_t> rootCodes;
    std::vector<RtModel> hModels;
    std::vector<RtSphere> hSpheres;
    int nTris = 0, maxHeight = 1;
    const RtTriangle* srcTris = nullptr; /* the caller's triangles: valid only while the call that prepared the scene runs (commit_scene keeps their corners) */
    bool flat = true;
    int wavesPerGroup = 1; /* plan_groups: what the layout's cache prefix was sized for */
    std::string error;     /* prepare_scene refused the scene: why */
};

/* Formats a refusal into `msg` (the 512 bytes a context keeps of it) and returns `status` */
__attribute__((format(printf, 3, 4))) static inline int prepare_fail(std::string& msg, int status, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    msg = buf;
    return status;
}

/* returns the status; a refusal's message is left in ps.error (the caller reports it on its context) */
static inline int prepare_scene(const RtModel* models, int n_models, const RtTriangle* triangles, int n_triangles,
                                const RtBVHNode* nodes, int n_nodes, const RtSphere* spheres, int n_spheres, PreparedScene& ps, const char* layoutOverride = nullptr)
{
    if (n_models < 0 || n_triangles < 0 || n_nodes < 0 || n_spheres < 0 || (n_models && !models) || (n_triangles && !triangles) ||
        (n_nodes && !nodes) || (n_spheres && !spheres))
        return prepare_fail(ps.error, RT_ERR_INVALID_ARG, "rt_upload_scene: bad pointer/count");

    /* ---- validate + re-lay out the BVHs reachable from the models */
    SceneBuilder sb;
    sb.nodes = nodes;
    sb.nNodes = n_nodes;
    sb.nTris = n_triangles;
    std::vector<uint32_t>& rootCodes = ps.rootCodes;
    std::vector<RtBVHNode>& rootChildren = ps.rootChildren;
    rootCodes.assign(n_models, 0u);
    rootChildren.assign((size_t)n_models * 2, RtBVHNode());
    std::vector<int> heights(n_models, 0);
    for (int i = 0; i < n_models; i++) {
        const RtModel& m = models[i];
        if (m.nodeOffset < 0 || m.nodeOffset >= n_nodes || m.triOffset < 0 || m.triOffset > n_triangles)
            return prepare_fail(ps.error, RT_ERR_SCENE, "model %d: nodeOffset/triOffset out of range", i);
        if (nodes[m.nodeOffset].triangleCount == 0)
            return prepare_fail(ps.error, RT_ERR_SCENE, "model %d: root node has triangleCount 0 (empty mesh) — undefined in the reference (RC:246)", i);
    }
    /* the distinct meshes (by root node), in the order the models name them */
    struct MeshJob { int nodeOffset, triOffset, firstModel; size_t segStart = 0; SceneBuilder sb; uint32_t code = 0; int height = 0; long long leafEnd = 0; bool ok = false; };
    std::vector<MeshJob> jobs;
    std::vector<int> jobOfModel(n_models, 0);
    {
        std::unordered_map<int, int> jobOfRoot; /* (a scene of 10^5 models with a mesh each must not pay 10^10 comparisons here) */
        for (int i = 0; i < n_models && jobs.size() <= 256; i++) { /* more than 256 meshes: the sequential walk below, no jobs needed */
            auto it = jobOfRoot.find(models[i].nodeOffset);
            if (it == jobOfRoot.end()) {
                it = jobOfRoot.emplace(models[i].nodeOffset, (int)jobs.size()).first;
                jobs.emplace_back();
                jobs.back().nodeOffset = models[i].nodeOffset; jobs.back().triOffset = models[i].triOffset; jobs.back().firstModel = i;
            }
            jobOfModel[i] = it->second;
        }
    }
    bool merged = false;
    size_t nPairs = 0;
    if (jobs.size() >= 2 && jobs.size() <= 256 && n_nodes >= (1 << 16) && !getenv("RT_SEQUENTIAL_PREPARE")) {
        /* large scene with several meshes: one worker per mesh.  A mesh's nodes are expected in the window from its root to the next
         * mesh's root (how CreateAllMeshData lays them out, RCM:206-236); a window of w nodes holds at most w / 2 pairs, so every mesh
         * gets its segment of ONE uninitialised pair array up front and writes final ids — nothing is merged or rebased. */
        std::vector<int> order(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) order[j] = (int)j;
        std::sort(order.begin(), order.end(), [&](int x, int y) { return jobs[x].nodeOffset < jobs[y].nodeOffset; });
        std::vector<size_t> segStart(jobs.size() + 1, 0);
        std::vector<int> winEnd(jobs.size(), n_nodes);
        for (size_t k = 0; k < order.size(); k++) {
            const int j = order[k];
            winEnd[j] = k + 1 < order.size() ? jobs[order[k + 1]].nodeOffset : n_nodes;
            jobs[j].segStart = segStart[k];
            segStart[k + 1] = segStart[k] + (size_t)(winEnd[j] - jobs[j].nodeOffset) / 2 + 1;
        }
        if (segStart[order.size()] < ((size_t)1 << 26) && ps.pairs.resize_uninit(segStart[order.size()])) {
            parallel_jobs((int)jobs.size(), [&](int j) {
                MeshJob& mj = jobs[j];
                mj.sb.nodes = nodes; mj.sb.nNodes = n_nodes; mj.sb.nTris = n_triangles;
                mj.sb.memoLo = mj.nodeOffset;
                mj.sb.pairOfFirstChild.assign((size_t)(winEnd[j] - mj.nodeOffset) + 1, -1);
                mj.sb.seg = ps.pairs.data() + mj.segStart;
                mj.sb.segCap = (size_t)(winEnd[j] - mj.nodeOffset) / 2 + 1;
                mj.sb.idBase = (uint32_t)mj.segStart;
                mj.sb.pairDepth.reserve(mj.sb.segCap);
                mj.sb.pairLeafEnd.reserve(mj.sb.segCap);
                mj.ok = mj.sb.convert(mj.nodeOffset, mj.triOffset, mj.nodeOffset, &mj.code, &mj.height, &mj.leafEnd);
                memset(static_cast<void*>(mj.sb.seg + mj.sb.segCount), 0, (mj.sb.segCap - mj.sb.segCount) * sizeof(DPair)); /* the unused tail of the segment */
            });
            merged = true;
            for (const MeshJob& mj : jobs)
                if (mj.sb.outside || !mj.sb.bigLeaves.empty()) merged = false; /* (oversized leaves index a table the meshes would share) */
        }
    }
    if (merged) {
        for (int i = 0; i < n_models; i++) { /* errors in model order, as the sequential walk reports them */
            const MeshJob& mj = jobs[jobOfModel[i]];
            if (!mj.ok) return prepare_fail(ps.error, RT_ERR_SCENE, "model %d: %s", i, mj.sb.error.c_str());
            if ((long long)models[i].triOffset + mj.leafEnd > n_triangles) return prepare_fail(ps.error, RT_ERR_SCENE, "model %d: leaf triangle range out of bounds", i);
            rootCodes[i] = mj.code;
            heights[i] = mj.height;
        }
        for (const MeshJob& mj : jobs)
            if (mj.segStart + mj.sb.segCount > nPairs) nPairs = mj.segStart + mj.sb.segCount;
        ps.pairs.shrink(nPairs);
        jobs.clear();
    } else {
        jobs.clear();
        sb.pairOfFirstChild.assign((size_t)n_nodes + 1, -1);
        for (int i = 0; i < n_models; i++) {
            const RtModel& m = models[i];
            if (!sb.convert(m.nodeOffset, m.triOffset, m.nodeOffset, &rootCodes[i], &heights[i]))
                return prepare_fail(ps.error, RT_ERR_SCENE, "model %d: %s", i, sb.error.c_str());
        }
        nPairs = sb.pairs.size();
        if (nPairs < ((size_t)1 << 26)) {
            if (!ps.pairs.resize_uninit(nPairs)) return prepare_fail(ps.error, RT_ERR_OOM, "rt_upload_scene: out of host memory");
            if (nPairs) memcpy(static_cast<void*>(ps.pairs.data()), sb.pairs.data(), nPairs * sizeof(DPair));
        }
        std::vector<DPair>().swap(sb.pairs);
    }
    int maxHeight = 1;
    for (int i = 0; i < n_models; i++) {
        const RtModel& m = models[i];
        const RtBVHNode& root = nodes[m.nodeOffset];
        const int height = heights[i];
        if (height > RT_MAX_BVH_DEPTH) return prepare_fail(ps.error, RT_ERR_SCENE, "model %d: BVH depth %d > %d", i, height, RT_MAX_BVH_DEPTH);
        if (height > maxHeight) maxHeight = height;
        if (!(rootCodes[i] & RT_CODE_LEAF)) {
            rootChildren[2 * (size_t)i] = nodes[m.nodeOffset + root.startIndex];
            rootChildren[2 * (size_t)i + 1] = nodes[m.nodeOffset + root.startIndex + 1];
        } else { /* leaf root: the bounds of its triangles (validated by leaf_code above), count in triangleCount */
            RtBVHNode b;
            memset(&b, 0, sizeof(b));
            for (int d = 0; d < 3; d++) { b.boundsMin[d] = INFINITY; b.boundsMax[d] = -INFINITY; }
            bool fin = true;
            for (int t = 0; t < root.triangleCount; t++) {
                const RtTriangle& tr = triangles[(size_t)m.triOffset + root.startIndex + t];
                const float* vs[3] = {tr.posA, tr.posB, tr.posC};
                for (int v = 0; v < 3; v++)
                    for (int d = 0; d < 3; d++) {
                        fin = fin && std::isfinite(vs[v][d]);
                        b.boundsMin[d] = fminf(b.boundsMin[d], vs[v][d]);
                        b.boundsMax[d] = fmaxf(b.boundsMax[d], vs[v][d]);
                    }
            }
            b.triangleCount = (fin && root.triangleCount < (1 << 23)) ? root.triangleCount : 0; /* 0 = never filtered */
            rootChildren[2 * (size_t)i] = b;
            rootChildren[2 * (size_t)i + 1] = b;
        }
    }

    const auto tConv = std::chrono::steady_clock::now();
    /* the kernels address pairs and triangles with 32-bit byte offsets from the array bases (rt_kernels.h) */
    if (nPairs >= ((size_t)1 << 26) || (size_t)n_triangles * sizeof(DTri) >= ((size_t)1 << 32))
        return prepare_fail(ps.error, RT_ERR_SCENE, "scene too large for 32-bit offsets: %zu node pairs (limit 2^26), %d triangles (limit 2^32 / 48)", nPairs, n_triangles);

    /* ---- the layout: canonical pairs + the caller's triangles -> the pair / triangle / normal spaces the kernels address in
     * 16-byte units (rt_layout.h); triangles are pre-differenced on the way (RC:190-192 are ray independent, same fp32 ops) */
    {
        RtLayout L;
        const char* want = layoutOverride ? layoutOverride : getenv("RT_LAYOUT");
        if (!parse_layout(want ? want : RT_LAYOUT_DEFAULT, &L)) return prepare_fail(ps.error, RT_ERR_INVALID_ARG, "RT_LAYOUT=%s: unknown layout", want ? want : RT_LAYOUT_DEFAULT);
        {   /* the top-of-tree cache: as many records as the workgroups' LDS holds (or what RT_LAYOUT's cache=N says, within that) */
            bool anyInner = false;
            for (int i = 0; i < n_models; i++) anyInner = anyInner || !(rootCodes[i] & RT_CODE_LEAF);
            const char* wantWaves = getenv("RT_WAVES_PER_GROUP");
            const char* hotKB = getenv("RT_HOT_KB");
            const rt_plan::GroupPlan gp = anyInner ? rt_plan::plan_groups(maxHeight, n_models, wantWaves ? atoi(wantWaves) : RT_MAX_WAVES_PER_GROUP, hotKB != nullptr,
                                                                           hotKB ? atoll(hotKB) : 0)
                                                   : rt_plan::GroupPlan();
            ps.wavesPerGroup = gp.wavesPerGroup;
            /* Default rule (no `cache` word): the cache is used where it was measured to pay — scenes whose trees are small enough that the
             * records the LDS holds are at least 1/16 of all node pairs (configs 3 and 6: 96 % / 73 % of the inner steps served, frame time
             * 0 / - 1.1 % against the single-wave kernel; config 4 / 5 with 0.2 % / 0.01 % coverage: 63 % / 39 % served, + 3.6 % / - 0.3 %:
             * profiles/r06_groups_and_streams.txt).  Without it the BVH variants are round 5's single-wave workgroups on two streams. */
            if (L.cacheRecords == -1) L.cacheRecords = ((size_t)gp.cacheRecords * 16 >= nPairs) ? gp.cacheRecords : 0;
            if (L.cacheRecords < 0 || L.cacheRecords > gp.cacheRecords) L.cacheRecords = gp.cacheRecords;
            if (L.dense()) L.cacheRecords = 0; /* the dense layout moves nothing */
        }
        LayoutEngine eng;
        eng.canon = ps.pairs.data();
        eng.nCanon = nPairs;
        eng.canonBig = &sb.bigLeaves;
        eng.models = models;
        eng.nModels = n_models;
        eng.rootCodes = rootCodes.data();
        eng.tris = triangles;
        eng.nTris = n_triangles;
        eng.parallel = [](int n, void* c, void (*f)(void*, int)) { parallel_jobs(n, [&](int k) { f(c, k); }); };
        if (!eng.run(L, ps.pairs, ps.lay)) {
            const bool oom = ps.lay.error == "out of host memory";
            return prepare_fail(ps.error, oom ? RT_ERR_OOM : RT_ERR_SCENE, "rt_upload_scene: %s", ps.lay.error.c_str());
        }
        ps.nPairs = nPairs;
        rootCodes = ps.lay.rootCodes; /* final codes from here on (only their leaf bit is read below) */
    }
    if (getenv("RT_DEBUG_UPLOAD"))
        fprintf(stderr, "[rt] prepare_scene: layout %s (%zu + %zu + %zu bytes) in %.2f ms\n", ps.lay.used.name().c_str(), ps.lay.pairBuf.size(), ps.lay.triBuf.size(),
                ps.lay.normBuf.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tConv).count());
    pack_spheres(spheres, n_spheres, ps.sph, &ps.sphereBound);
    ps.mats.resize((size_t)n_spheres + n_models);
    for (int i = 0; i < n_spheres; i++) pack_material(spheres[i].material, ps.mats[i]);
    ps.dmodels.resize(n_models);
    for (int i = 0; i < n_models; i++) {
        pack_model(models[i], rootCodes[i], ps.lay.triBase[i], ps.dmodels[i]);
        pack_material(models[i].material, ps.mats[n_spheres + i]);
    }
    make_filters(models, n_models, rootCodes, rootChildren, spheres, n_spheres, ps.filters, &ps.maxOrigin);
    make_chunks(ps.filters, ps.chunks, &ps.nFiltered, &ps.extWords);
    ps.filters = append_filter_pairs(ps.filters); /* uploaded as one array */
    ps.hModels.assign(models, models + n_models);
    ps.hSpheres.assign(spheres, spheres + n_spheres);
    ps.nTris = n_triangles;
    ps.srcTris = triangles;
    ps.maxHeight = maxHeight;
    ps.flat = true;
    for (int i = 0; i < n_models; i++)
        if (!(rootCodes[i] & RT_CODE_LEAF)) ps.flat = false;
    return RT_OK;
}

#endif
