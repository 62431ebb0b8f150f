/*
 * rt_tile_cand.h — the per-TILE sphere candidates of the FLAT trace kernel's all-camera-ray waves (internal; plain C++, no HIP).
 *
 * Without defocus every camera ray of a pixel runs from camOrigin through focusPoint(pixel) + jitter (trace_body, RC:565-576), so which
 * spheres the 2,048 camera rays of an 8 x 8 tile's item can be accepted by depends on the tile, the camera and the spheres, not on the
 * ray.  tile_cand_mask decides it once per tile, conservatively; a wave that holds nothing but fresh camera rays (rt_primary.h) reads
 * its lanes' masks from a table instead of running the per-ray pre-test of begin_intersect.  The exact test behind the mask is unchanged:
 * the mask only has to hold every sphere whose exact test ACCEPTS a ray (disc >= 0 and dstFar >= 0, RC:304-312) — a sphere behind the
 * camera, whose whole line has a discriminant but whose roots are negative, may be dropped.
 *
 * The geometry (o = camOrigin, R / U / F = the camera's first three columns):
 *   focusPoint(x, y) = o + R fx(x) + U fy(y) + F vz is affine in (x, y), so every point the rays of the tile's pixels are aimed at lies
 *   in the ball B(Pc, Rt): Pc = focusPoint(tile centre), Rt = the farthest corner of a rectangle of 4 pixels (not 3.5) to either side
 *   plus the jitter bound diverge rcpW (|R| + |U|).  Every ray direction therefore lies in the cone of half-angle alpha around
 *   a = Pc - o with sin(alpha) = Rt / |a|.
 *   A ray from o that the exact test of sphere (c, r) accepts goes FORWARD to within r' of c, so it lies in the cone of half-angle beta
 *   around v = c - o with sin(beta) = r' / |v| (o outside the sphere).
 *   If the angle between a and v exceeds alpha + beta < 90 degrees the two cones share no direction: the bit is clear.
 * Why this is conservative in fp32 — three lines instead of an error analysis:
 *   1. Every radius (Rt, r') and then every sine is inflated by 1 %, four orders of magnitude above the rounding of the few fp32 operations
 *      here and in the raygen (2^-24 per operation), and both radii get 2^-16 of the scale |o| + |Pc| + |c| + r added: the rounding of
 *      o - c, of focusPoint and of the jitter is relative to the COORDINATES, not to the distances.
 *   2. The exact test's discriminant carries a rounding error of at most 2^-24 (d.d)(21 |o-c|^2 + 11 r^2) (begin_intersect), so it accepts
 *      rays that pass within sqrt(r^2 + E) of c: r'^2 = r^2 + 2^-17 (|o-c|^2 + r^2) covers E six times over.
 *   3. Everything that is not clearly inside these assumptions keeps the sphere: o inside or near it (sin(beta) >= 1), a degenerate cone
 *      (|a| <= Rt: sin(alpha) >= 1), alpha + beta near 90 degrees or beyond (sin^2(alpha) + sin^2(beta) >= 0.98), any value that is not
 *      finite.  The angles are compared through the cross product (sines), which keeps its relative accuracy for small angles.
 * tests/tile_cand_driver.cpp is the proof by exhaustion: the kernel's own raygen formulas, the exact test, 0 misses.
 *
 * The per-tile TRIANGLE candidates (tile_tri_mask; FLAT scenes within the caps of rt_primary.h): one bit per root-leaf triangle, in the
 * order traverse_flat meets them.  A bit may be clear only when no camera ray of the tile can satisfy dst > 0 && u >= 0 && v >= 0 && w >= 0
 * in tri_test's own arithmetic (the keep / cull condition is ignored: that keeps more).  With the table's p = lpos - A and e = dot(p, face),
 * and for a local direction d, tri_test forms det = -d.face, U = d.(AC x p), V = d.(p x AB) and accepts only if e / det > 0, U / det >= 0,
 * V / det >= 0 and 1 - U / det - V / det >= 0.  With s = sign(e) that needs s det > 0, s U >= 0, s V >= 0 and s (det - U - V) >= 0: four
 * functions LINEAR in d, taken from the very records the kernel reads (w2l, the table's lpos, A, edgeAB, edgeAC and the stored face — not
 * l2w, not a recomputed normal, no assumption on winding or on the sign of w2l's determinant).
 *   Every unnormalised direction o -> target of the tile is R s + U t + F vz with (s, t) in a rectangle: 4 pixels to either side of the
 *   tile's centre plus the jitter bound, as above.  It is a convex combination of the rectangle's four corners g_j, w2l's 3 x 3 part is
 *   linear and normalising scales by a positive number, so a function that is negative at all four corners is negative for every ray.
 * Why this is conservative in fp32:
 *   1. A function counts as negative only below -2^-14 N |w2l| (|o| + max |g_j|), N = (|lpos| + |A|) |edge| resp. |face| resp. their sum
 *      bounding the normal: the rounding of the raygen, of w2l x d and of tri_test's products is 2^-24 per operation relative to the
 *      COORDINATES (|o| + |target|, |lpos| + |A|), a thousand times less.
 *   2. Everything that is not clearly inside these assumptions keeps the triangle: W or H of 1, any value that is not finite, lengths
 *      outside 2^-16 ... 2^16 (no product may leave fp32's normal range), e within the margin of 0 (lpos in the plane or on a vertex),
 *      a normal within the margin of 0 (lpos on an edge line, a degenerate triangle), corners on both sides of a plane.
 * tests/tile_tri_driver.cpp is the proof by exhaustion, as for the spheres.
 */
#ifndef RT_TILE_CAND_H
#define RT_TILE_CAND_H

#include <stdint.h>
#include <string.h>

#include "../../include/rt_math.h"

#define RT_TILE_CAND_MAX_SPHERES 32 /* one mask word = one 32-sphere block of begin_intersect (== RT_PRIMARY_MAX_SPHERES) */
#define RT_TILE_TRI_MAX_MODELS 4    /* == RT_PRIMARY_MAX_MODELS */
#define RT_TILE_TRI_MAX_TRIS 16     /* == RT_PRIMARY_MAX_TRIS */

/* What the masks of a context's tiles depend on, and nothing else: the argument block of the fill kernel, passed by value, and at the
 * same time the KEY of a filled table (compared bytewise: make it with tile_cand_key_init, which clears the padding).  The camera fields
 * are those the refill and raygen blocks of trace_body read; the spheres are pack_spheres' exact records (centre, r*r). */
struct TileCandKey {
    float cam[16];
    float viewParams[3];
    float rcpWm1, rcpHm1, rcpW, diverge;
    float camOrigin[3];
    int32_t W, H;                               /* (part of the key only: rcpWm1, rcpHm1 and rcpW are what the geometry reads) */
    int32_t tilesX, tiles;                      /* this context's tiles: tilesX per row of tiles, `tiles` in all = entries of the table */
    int32_t stripRows, partIndex, partCount;    /* local tile row -> global row, as RT_SET_POOL of trace_body */
    int32_t nSpheres;
    float sph[RT_TILE_CAND_MAX_SPHERES][4];
    /* the triangle half (tile_tri_mask); triOn = 0: not in use, the fill kernel writes all ones */
    int32_t triOn;
    int32_t nTriModels;
    int32_t triCount[RT_TILE_TRI_MAX_MODELS];   /* root-leaf triangles per model, as primary_collect_tris decodes them */
    float w2l[RT_TILE_TRI_MAX_MODELS][12];      /* DModel::w2l: what traverse_flat multiplies the direction with */
    float lpos[RT_TILE_TRI_MAX_MODELS][4];      /* PrimaryTable::lpos */
    float tri[RT_TILE_TRI_MAX_TRIS][12];        /* (A, edgeAB, edgeAC, face) of the laid-out record, local space, in traverse_flat's order */
};

static inline void tile_cand_key_init(TileCandKey& k) { memset(&k, 0, sizeof(k)); }

/* first column and first GLOBAL row of local tile `tile` (RT_SET_POOL: cyclic strips, every row of a tile in one strip) */
RT_HD void tile_cand_origin(const TileCandKey& k, int tile, int* x0, int* y0)
{
    const int ty = tile / k.tilesX;
    const int row0 = ty * 8;
    const int ls = row0 / k.stripRows;
    *x0 = (tile - ty * k.tilesX) * 8;
    *y0 = (ls * k.partCount + k.partIndex) * k.stripRows + (row0 - ls * k.stripRows);
}

RT_HD bool tile_cand_finite(float x) { return rt_abs(x) < RT_INF; } /* false for NaN */

/* Bit s set: sphere s may be accepted by a camera ray of a pixel of the tile whose first column / global row are (x0, y0). */
RT_HD uint32_t tile_cand_mask(const TileCandKey& k, int x0, int y0)
{
    const int n = k.nSpheres < RT_TILE_CAND_MAX_SPHERES ? k.nSpheres : RT_TILE_CAND_MAX_SPHERES;
    const uint32_t all = n >= 32 ? 0xffffffffu : ((1u << (n > 0 ? n : 0)) - 1u);
    const float slack = 1.01f;
    const rt_f3 o = rt_v3(k.camOrigin[0], k.camOrigin[1], k.camOrigin[2]);
    const rt_f3 R = rt_v3(k.cam[0], k.cam[1], k.cam[2]), U = rt_v3(k.cam[4], k.cam[5], k.cam[6]), F = rt_v3(k.cam[8], k.cam[9], k.cam[10]);
    /* a = Pc - o, without the cancellation of forming Pc first: the tile centre is pixel (x0 + 3.5, y0 + 3.5) */
    const float fx = (((float)x0 + 3.5f) * k.rcpWm1 - 0.5f) * k.viewParams[0];
    const float fy = (((float)y0 + 3.5f) * k.rcpHm1 - 0.5f) * k.viewParams[1];
    const rt_f3 a = R * fx + U * fy + F * k.viewParams[2];
    const float lenR = rt_sqrt(rt_dot(R, R)), lenU = rt_sqrt(rt_dot(U, U));
    /* the rectangle's half-extents along R and U, and its farthest corner: |hx R^ +- hy U^|^2 = hx^2 + hy^2 + 2 hx hy |R^.U^| */
    const float ex = 4.0f * rt_abs(k.rcpWm1 * k.viewParams[0]), ey = 4.0f * rt_abs(k.rcpHm1 * k.viewParams[1]);
    const float hx = ex * lenR, hy = ey * lenU;
    const float corner = rt_sqrt(hx * hx + hy * hy + 2.0f * ex * ey * rt_abs(rt_dot(R, U)));
    const float jitter = rt_abs(k.diverge * k.rcpW) * (lenR + lenU);
    const float L2 = rt_dot(a, a);
    const float lenO = rt_sqrt(rt_dot(o, o)), lenPc = lenO + rt_sqrt(L2); /* >= |Pc| */
    if (!(tile_cand_finite(corner) && tile_cand_finite(jitter) && tile_cand_finite(lenPc) && L2 > 0.0f)) return all;
    uint32_t mask = 0;
    for (int s = 0; s < n; s++) {
        const rt_f3 v = rt_v3(k.sph[s][0], k.sph[s][1], k.sph[s][2]) - o;
        const float rr = k.sph[s][3];
        const float D2 = rt_dot(v, v);
        const float scale = 1.52587890625e-05f * (lenO + lenPc + (lenO + rt_sqrt(D2)) + rt_sqrt(rt_abs(rr))); /* 2^-16 (|o| + |Pc| + |c| + r), from above */
        const float Rt = slack * (corner + jitter) + scale;
        const float re = slack * rt_sqrt(rr + 7.62939453125e-06f * (D2 + rr)) + scale; /* r' of 2. above */
        const float sa2 = slack * slack * (Rt * Rt) / L2, sb2 = slack * slack * (re * re) / D2; /* the inflated sines, squared */
        const rt_f3 cr = rt_cross(a, v);
        const float cross2 = rt_dot(cr, cr), av = rt_dot(a, v);
        const float lim = L2 * D2;
        bool drop = false;
        if (tile_cand_finite(sa2) && tile_cand_finite(sb2) && tile_cand_finite(cross2) && tile_cand_finite(av) && tile_cand_finite(lim) && sa2 + sb2 < 0.98f) {
            /* alpha + beta < 90 degrees.  sin(alpha + beta) = sa cb + ca sb; the angle between a and v is at least 90 degrees (a.v <= 0)
             * or has sin^2 = |a x v|^2 / (|a|^2 |v|^2) */
            const float sg = rt_sqrt(sa2) * rt_sqrt(1.0f - sb2) + rt_sqrt(1.0f - sa2) * rt_sqrt(sb2);
            drop = (av <= 0.0f) || (cross2 > sg * sg * lim);
        }
        if (!drop) mask |= 1u << s;
    }
    return mask;
}

/* Bit i set: the i-th root-leaf triangle traverse_flat meets may be accepted by a camera ray of a pixel of the tile at (x0, y0). */
RT_HD uint32_t tile_tri_mask(const TileCandKey& k, int x0, int y0)
{
    const int nm = k.nTriModels < RT_TILE_TRI_MAX_MODELS ? k.nTriModels : RT_TILE_TRI_MAX_MODELS;
    int n = 0;
    for (int m = 0; m < nm; m++) n += k.triCount[m] > 0 ? k.triCount[m] : 0;
    if (n > RT_TILE_TRI_MAX_TRIS) n = RT_TILE_TRI_MAX_TRIS;
    const uint32_t all = (1u << n) - 1u;
    if (k.W <= 1 || k.H <= 1) return all;
    const float eps = 6.103515625e-05f; /* 2^-14 */
    const float lo = 1.52587890625e-05f, hi = 65536.0f; /* 2^-16, 2^16 */
    const rt_f3 o = rt_v3(k.camOrigin[0], k.camOrigin[1], k.camOrigin[2]);
    const rt_f3 R = rt_v3(k.cam[0], k.cam[1], k.cam[2]), U = rt_v3(k.cam[4], k.cam[5], k.cam[6]), F = rt_v3(k.cam[8], k.cam[9], k.cam[10]);
    const float fx = (((float)x0 + 3.5f) * k.rcpWm1 - 0.5f) * k.viewParams[0];
    const float fy = (((float)y0 + 3.5f) * k.rcpHm1 - 0.5f) * k.viewParams[1];
    const float jit = 1.01f * rt_abs(k.diverge * k.rcpW);
    const float ex = 4.0f * rt_abs(k.rcpWm1 * k.viewParams[0]) + jit, ey = 4.0f * rt_abs(k.rcpHm1 * k.viewParams[1]) + jit;
    rt_f3 g[4];
    float gmax = 0.0f;
    for (int j = 0; j < 4; j++) {
        g[j] = F * k.viewParams[2] + R * ((j & 1) ? fx + ex : fx - ex) + U * ((j & 2) ? fy + ey : fy - ey);
        const float len = rt_sqrt(rt_dot(g[j], g[j]));
        if (!tile_cand_finite(len)) return all;
        gmax = rt_max(gmax, len);
    }
    const float lenO = rt_sqrt(rt_dot(o, o));
    if (!(tile_cand_finite(lenO) && lenO <= hi && gmax >= lo && gmax <= hi)) return all;
    uint32_t mask = 0;
    int t = 0;
    for (int m = 0; m < nm; m++) {
        const float* w = k.w2l[m];
        const float wn = rt_abs(w[0]) + rt_abs(w[1]) + rt_abs(w[2]) + rt_abs(w[4]) + rt_abs(w[5]) + rt_abs(w[6]) + rt_abs(w[8]) + rt_abs(w[9]) + rt_abs(w[10]);
        rt_f3 c[4];
        for (int j = 0; j < 4; j++)
            c[j] = rt_v3(w[0] * g[j].x + w[1] * g[j].y + w[2] * g[j].z, w[4] * g[j].x + w[5] * g[j].y + w[6] * g[j].z, w[8] * g[j].x + w[9] * g[j].y + w[10] * g[j].z);
        const float dirScale = wn * (lenO + gmax); /* bounds |w2l x (o -> target)| and the coordinates its rounding is relative to */
        const rt_f3 lpos = rt_v3(k.lpos[m][0], k.lpos[m][1], k.lpos[m][2]);
        const float lenL = rt_sqrt(rt_dot(lpos, lpos));
        const bool modelOk = wn >= lo && wn <= hi && tile_cand_finite(lenL);
        for (int i = 0; i < k.triCount[m] && t < n; i++, t++) {
            const float* q = k.tri[t];
            const rt_f3 A = rt_v3(q[0], q[1], q[2]), AB = rt_v3(q[3], q[4], q[5]), AC = rt_v3(q[6], q[7], q[8]), face = rt_v3(q[9], q[10], q[11]);
            const rt_f3 p = lpos - A; /* tri_test's vertRayOffset, as primary_fill forms it */
            const float e = rt_dot(p, face);
            const float lenP = lenL + rt_sqrt(rt_dot(A, A));
            const float nab = rt_sqrt(rt_dot(AB, AB)), nac = rt_sqrt(rt_dot(AC, AC)), nf = rt_sqrt(rt_dot(face, face));
            const float NU = lenP * nac, NV = lenP * nab, ND = nf, NW = ND + NU + NV;
            bool drop = false;
            if (modelOk && lenP >= lo && lenP <= hi && nab >= lo && nab <= hi && nac >= lo && nac <= hi && nf >= lo * lo && nf <= hi * hi &&
                tile_cand_finite(e) && rt_abs(e) > eps * lenP * nf) {
                const float s = e > 0.0f ? 1.0f : -1.0f;
                const rt_f3 nD = face * (-s), nU = rt_cross(AC, p) * s, nV = rt_cross(p, AB) * s, nW = nD - nU - nV;
                const rt_f3 nrm[4] = {nD, nU, nV, nW};
                const float bound[4] = {ND, NU, NV, NW};
                bool sound = true;
                for (int f = 0; f < 4; f++) { /* a normal within the margin of zero: lpos on an edge line, a degenerate triangle */
                    const float l2 = rt_dot(nrm[f], nrm[f]), z = eps * bound[f];
                    sound = sound && tile_cand_finite(l2) && l2 > z * z;
                }
                for (int f = 0; f < 4 && sound && !drop; f++) {
                    const float margin = eps * bound[f] * dirScale;
                    bool out = tile_cand_finite(margin);
                    for (int j = 0; j < 4; j++) out = out && rt_dot(nrm[f], c[j]) < -margin; /* (false for NaN) */
                    drop = out;
                }
            }
            if (!drop) mask |= 1u << t;
        }
    }
    return mask | (all & ~((t >= 32 ? 0u : (1u << t)) - 1u)); /* (triangles the loop did not reach stay set) */
}

#endif
