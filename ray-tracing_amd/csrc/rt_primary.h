/*
 * rt_primary.h — the per-launch table of RAY-ORIGIN CONSTANTS of the FLAT trace kernel (internal; plain C++, no HIP).
 *
 * Without defocus every camera ray of a launch starts at ONE point, camOrigin, and two segments in three of the headline scene are
 * camera rays.  The terms of the intersection that depend only on the ray origin and the scene — |o|^2, c.o per sphere, o - c, the
 * origin in each model's local space, o' - A per triangle — are then the same values in every lane of every wave.  primary_fill
 * computes them once per launch on the host, with the very fp32 operations, in the very order, the kernel performs per ray
 * (begin_intersect, traverse_flat, tri_test in rt_kernels.h; include/rt_math.h for the strict forms), so a wave whose active lanes
 * are all fresh camera rays may read them instead: same bits.  tests/primary_driver.cpp compares every entry with the per-ray formula.
 *
 * The table travels by value at the end of the kernel arguments (rt_device.h): a launch in flight never sees it change.
 */
#ifndef RT_PRIMARY_H
#define RT_PRIMARY_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/rt_math.h"
#include "rt_records.h"

/* the caps: one 32-sphere block of the pre-test, and what a scalar-loaded table may reasonably hold */
#define RT_PRIMARY_MAX_SPHERES 32
#define RT_PRIMARY_MAX_MODELS 4
#define RT_PRIMARY_MAX_TRIS 16

struct alignas(16) PrimaryTable {
    int32_t on;          /* 0: the kernel computes everything per ray, as it always did (camOrigin below stays valid) */
    float ooBound;       /* |o|^2 + sphereBound: the pre-test's margin is -(2^-17 (d.d) ooBound) */
    int32_t pad[2];
    float camOrigin[4];  /* rt_mul_point(cam, 0, 1) — what the raygen block reads when raygenNoDefocus is set */
    float lpos[RT_PRIMARY_MAX_MODELS][4];         /* worldToLocal x camOrigin per model */
    float pair[RT_PRIMARY_MAX_SPHERES / 2][8];    /* (cx0, cx1, cy0, cy1, cz0, cz1, ct0, ct1), ct = fma(-2, c.o, |o|^2) + K: the pre-test's pair record with K replaced */
    float sph[RT_PRIMARY_MAX_SPHERES][4];         /* (o - c, dot(o - c, o - c) - r*r): the exact test's per-origin terms */
    float tri[RT_PRIMARY_MAX_TRIS][4];            /* (o' - A, dot(o' - A, face)) per root-leaf triangle, in the order traverse_flat meets them */
};

/* What the table needs of a FLAT scene's triangles, taken from the laid-out triangle space ONCE per upload (matrices move with
 * rt_update_models, local-space triangles do not): A and face of every model's root leaf, in model order. */
struct PrimaryTris {
    bool usable = false; /* FLAT, within the caps, every record inside the triangle space */
    int nModels = 0;
    int count[RT_PRIMARY_MAX_MODELS] = {0, 0, 0, 0};
    float a[RT_PRIMARY_MAX_TRIS][3];
    float face[RT_PRIMARY_MAX_TRIS][3];
    float ab[RT_PRIMARY_MAX_TRIS][3];   /* edgeAB and edgeAC of the same records: what the per-tile triangle masks need besides (rt_tile_cand.h) */
    float ac[RT_PRIMARY_MAX_TRIS][3];
};

static inline void primary_collect_tris(bool flat, const DModel* models, int nModels, const unsigned char* triSpace, size_t triSpaceBytes,
                                        const uint32_t* bigLeaves, size_t nBigLeafWords, PrimaryTris& out)
{
    out = PrimaryTris();
    if (!flat || nModels < 0 || nModels > RT_PRIMARY_MAX_MODELS) return;
    int total = 0;
    for (int m = 0; m < nModels; m++) {
        /* the root leaf as traverse_flat decodes it */
        const uint32_t code = models[m].rootCode;
        uint32_t count = (code >> 24) & 0x7fu, start = code & RT_CODE_MAX_INLINE_START;
        if (count == 0) {
            if (2 * (size_t)start + 1 >= nBigLeafWords) return;
            count = bigLeaves[2 * (size_t)start + 1];
            start = bigLeaves[2 * (size_t)start];
        }
        if (count > (uint32_t)(RT_PRIMARY_MAX_TRIS - total)) return;
        for (uint32_t i = 0; i < count; i++) {
            const long long unit = (long long)models[m].triBase + (long long)start + 3ll * (long long)i;
            if (unit < 0 || ((size_t)unit + 3) * 16 > triSpaceBytes) return;
            DTri t;
            memcpy(&t, triSpace + (size_t)unit * 16, sizeof(t));
            out.a[total][0] = t.ax; out.a[total][1] = t.ay; out.a[total][2] = t.az;
            out.face[total][0] = t.fx; out.face[total][1] = t.fy; out.face[total][2] = t.fz;
            out.ab[total][0] = t.abx; out.ab[total][1] = t.aby; out.ab[total][2] = t.abz;
            out.ac[total][0] = t.acx; out.ac[total][1] = t.acy; out.ac[total][2] = t.acz;
            total++;
        }
        out.count[m] = (int)count;
    }
    out.nModels = nModels;
    out.usable = true;
}

/* May a launch carry the table at all?  (primary_fill still switches it off when an entry is not finite.)  switchOn = the context's
 * RT_PRIMARY; noDefocus = KArgs::raygenNoDefocus of the launch.  fill_args and tests/primary_driver.cpp both ask here. */
static inline bool primary_allowed(bool switchOn, bool noDefocus, bool flatScene, int nSpheres, int nModels, const PrimaryTris& tris)
{
    return switchOn && noDefocus && flatScene && nSpheres >= 0 && nSpheres <= RT_PRIMARY_MAX_SPHERES && nModels >= 0 && nModels <= RT_PRIMARY_MAX_MODELS &&
           tris.usable && tris.nModels == nModels;
}

/* camOrigin as the kernel's raygen block computes it */
static inline rt_f3 primary_cam_origin(const float* cam) { return rt_mul_point(cam, rt_v3(0.0f, 0.0f, 0.0f), 1.0f); }

/* Fills the table.  `allowed` = raygenNoDefocus && the run-time switch; sph = pack_spheres' array (nSpheres exact records, then the
 * pair records); w2l[m] = DModel::w2l of model m.  The table is switched on only when every entry is finite (a NaN has no agreed
 * bit pattern between the host and the device). */
static inline void primary_fill(PrimaryTable& t, bool allowed, rt_f3 camOrigin, const float* sph, int nSpheres, float sphereBound,
                                const DModel* models, int nModels, const PrimaryTris& tris)
{
    memset(&t, 0, sizeof(t));
    t.camOrigin[0] = camOrigin.x; t.camOrigin[1] = camOrigin.y; t.camOrigin[2] = camOrigin.z;
    if (!allowed || !tris.usable || tris.nModels != nModels || nSpheres < 0 || nSpheres > RT_PRIMARY_MAX_SPHERES) return;
    const rt_f3 o = camOrigin;
    bool fin = true;
    /* begin_intersect: oo, and the margin's sum */
    const float oo = __builtin_fmaf(o.x, o.x, __builtin_fmaf(o.y, o.y, o.z * o.z));
    t.ooBound = oo + sphereBound;
    fin = fin && std::isfinite(t.ooBound);
    /* the packed pre-test: co = fma(cx, ox, fma(cy, oy, cz * oz)), ct = fma(-2, co, oo) + K, both halves of a pair record */
    const float* sphq = sph + 4 * (size_t)nSpheres;
    for (int p = 0; p < (nSpheres + 1) / 2; p++) {
        const float* q = sphq + 8 * (size_t)p;
        float* r = t.pair[p];
        for (int h = 0; h < 2; h++) {
            const float cx = q[0 + h], cy = q[2 + h], cz = q[4 + h], kk = q[6 + h];
            const float co = __builtin_fmaf(cx, o.x, __builtin_fmaf(cy, o.y, cz * o.z));
            const float ct = __builtin_fmaf(-2.0f, co, oo) + kk;
            r[0 + h] = cx; r[2 + h] = cy; r[4 + h] = cz; r[6 + h] = ct;
            fin = fin && std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz) && std::isfinite(ct);
        }
    }
    /* the exact test: off = o - c, qc = dot(off, off) - r*r */
    for (int s = 0; s < nSpheres; s++) {
        const rt_f3 off = o - rt_v3(sph[4 * s + 0], sph[4 * s + 1], sph[4 * s + 2]);
        const float qc = rt_dot(off, off) - sph[4 * s + 3];
        t.sph[s][0] = off.x; t.sph[s][1] = off.y; t.sph[s][2] = off.z; t.sph[s][3] = qc;
        fin = fin && std::isfinite(off.x) && std::isfinite(off.y) && std::isfinite(off.z) && std::isfinite(qc);
    }
    /* traverse_flat: the origin in the model's space; tri_test: vertRayOffset and its dot with the face normal */
    int k = 0;
    for (int m = 0; m < nModels; m++) {
        const float* w = models[m].w2l;
        const rt_f3 lpos = rt_v3(w[0] * o.x + w[1] * o.y + w[2] * o.z + w[3] * 1.0f,
                                 w[4] * o.x + w[5] * o.y + w[6] * o.z + w[7] * 1.0f,
                                 w[8] * o.x + w[9] * o.y + w[10] * o.z + w[11] * 1.0f);
        t.lpos[m][0] = lpos.x; t.lpos[m][1] = lpos.y; t.lpos[m][2] = lpos.z;
        fin = fin && std::isfinite(lpos.x) && std::isfinite(lpos.y) && std::isfinite(lpos.z);
        for (int i = 0; i < tris.count[m]; i++, k++) {
            const rt_f3 vro = lpos - rt_v3(tris.a[k][0], tris.a[k][1], tris.a[k][2]);
            const float d = rt_dot(vro, rt_v3(tris.face[k][0], tris.face[k][1], tris.face[k][2]));
            t.tri[k][0] = vro.x; t.tri[k][1] = vro.y; t.tri[k][2] = vro.z; t.tri[k][3] = d;
            fin = fin && std::isfinite(vro.x) && std::isfinite(vro.y) && std::isfinite(vro.z) && std::isfinite(d);
        }
    }
    t.on = fin ? 1 : 0;
}

#endif
