/*
 * primary_driver.cpp — ray-tracing_amd/csrc/rt_primary.h on its own: seeded random cameras, spheres and leaf-root models go through the
 * real scene preparation (rt_scene_prep.h), the table of per-launch origin constants is filled, and every entry is compared BITWISE with
 * the per-ray formula of rt_kernels.h (begin_intersect, traverse_flat, tri_test) evaluated with include/rt_math.h at rpos = camOrigin.
 * tests/test_primary.py builds it plainly and with the address and undefined-behaviour sanitizers, as a stand-alone program.
 *
 * usage: primary_driver SEED CASES   -> "ok cases=N on=K" and exit 0, or "FAIL ..." lines and exit 1
 */
#include <stdio.h>
#include <stdlib.h>

#include <limits>

#include "../ray-tracing_amd/csrc/rt_scene_prep.h"
#include "../ray-tracing_amd/csrc/rt_primary.h"

static uint64_t g_state;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffff) / 16777216.0f; }
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)
static bool same(float a, float b) { return rt_f2u(a) == rt_f2u(b); }

struct Scene {
    std::vector<RtModel> models;
    std::vector<RtTriangle> tris;
    std::vector<RtBVHNode> nodes;
    std::vector<RtSphere> spheres;
};

/* a rigid-ish random affine matrix and its inverse are not needed exact: the table only reads worldToLocal */
static void random_matrix(float* m /* column-major */)
{
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) m[c * 4 + r] = (r == 3) ? (c == 3 ? 1.0f : 0.0f) : (c == 3 ? uni(-5, 5) : uni(-1.5f, 1.5f) + (r == c ? 2.0f : 0.0f));
}

/* nModels leaf-root models of trisPerModel triangles each (a quad is 2); `inner` gives model 0 an inner root instead (not FLAT) */
static Scene make_scene(int nSpheres, int nModels, const int* trisPerModel, bool inner)
{
    Scene s;
    for (int i = 0; i < nSpheres; i++) {
        RtSphere sp;
        memset(&sp, 0, sizeof(sp));
        for (int d = 0; d < 3; d++) sp.centre[d] = uni(-20, 20);
        sp.radius = uni(0.1f, 4);
        s.spheres.push_back(sp);
    }
    for (int m = 0; m < nModels; m++) {
        RtModel md;
        memset(&md, 0, sizeof(md));
        md.nodeOffset = (int)s.nodes.size();
        md.triOffset = (int)s.tris.size();
        random_matrix(md.worldToLocal);
        random_matrix(md.localToWorld);
        md.material.flag = (m & 1) ? RT_MATERIAL_GLASS : 0;
        const int n = trisPerModel[m];
        for (int t = 0; t < n; t++) {
            RtTriangle tr;
            memset(&tr, 0, sizeof(tr));
            for (int d = 0; d < 3; d++) { tr.posA[d] = uni(-3, 3); tr.posB[d] = uni(-3, 3); tr.posC[d] = uni(-3, 3); tr.normA[d] = tr.normB[d] = tr.normC[d] = d == 1; }
            s.tris.push_back(tr);
        }
        RtBVHNode root;
        memset(&root, 0, sizeof(root));
        for (int d = 0; d < 3; d++) { root.boundsMin[d] = -3; root.boundsMax[d] = 3; }
        if (inner && m == 0 && n >= 2) { /* root -> two leaves */
            root.startIndex = 1; root.triangleCount = -1; /* (0 at a root is refused as an empty mesh) */
            RtBVHNode a = root, b = root;
            a.startIndex = 0; a.triangleCount = 1;
            b.startIndex = 1; b.triangleCount = n - 1;
            s.nodes.push_back(root); s.nodes.push_back(a); s.nodes.push_back(b);
        } else {
            root.startIndex = 0; root.triangleCount = n;
            s.nodes.push_back(root);
        }
        s.models.push_back(md);
    }
    return s;
}

static void random_camera(float* cam)
{
    random_matrix(cam);
    for (int r = 0; r < 3; r++) cam[12 + r] = uni(-30, 30);
}

/* fill_args' rule for raygenNoDefocus (rt_context.hip) */
static bool no_defocus(const float* cam, float defocus, rt_f3 o)
{
    bool fin = true;
    for (int k = 0; k < 16; k++) fin = fin && std::isfinite(cam[k]);
    const bool noNegZero = rt_f2u(o.x) != 0x80000000u && rt_f2u(o.y) != 0x80000000u && rt_f2u(o.z) != 0x80000000u;
    return defocus == 0.0f && fin && noNegZero;
}

/* prepares the scene and fills the table as rt_context.hip does; returns false if the scene was refused */
static bool build(const Scene& s, const float* cam, float defocus, bool switchOn, PreparedScene& ps, PrimaryTris& pt, PrimaryTable& t)
{
    const int rc = prepare_scene(s.models.data(), (int)s.models.size(), s.tris.data(), (int)s.tris.size(), s.nodes.data(), (int)s.nodes.size(), s.spheres.data(),
                                 (int)s.spheres.size(), ps);
    if (rc != RT_OK) { printf("FAIL prepare_scene: %s\n", ps.error.c_str()); failures++; return false; }
    const auto& triSpace = ps.lay.arena ? ps.lay.pairBuf : ps.lay.triBuf;
    primary_collect_tris(ps.flat, ps.dmodels.data(), (int)ps.dmodels.size(), triSpace.data(), triSpace.size(), ps.lay.bigLeaves.data(), ps.lay.bigLeaves.size(), pt);
    const rt_f3 o = primary_cam_origin(cam);
    const bool allowed = primary_allowed(switchOn, no_defocus(cam, defocus, o), ps.flat, (int)s.spheres.size(), (int)s.models.size(), pt);
    primary_fill(t, allowed, o, ps.sph.data(), (int)s.spheres.size(), ps.sphereBound, ps.dmodels.data(), (int)ps.dmodels.size(), pt);
    CHECK(same(t.camOrigin[0], o.x) && same(t.camOrigin[1], o.y) && same(t.camOrigin[2], o.z), "camOrigin is always filled");
    return true;
}

/* every entry against the kernel's per-ray formula at rpos = camOrigin */
static void verify(const Scene& s, const float* cam, const PreparedScene& ps, const PrimaryTable& t, int id)
{
    const rt_f3 rpos = rt_mul_point(cam, rt_v3(0.0f, 0.0f, 0.0f), 1.0f);
    const int n = (int)s.spheres.size();
    const float* sph = ps.sph.data();
    const float* sphq = sph + 4 * (size_t)n;
    /* begin_intersect */
    const float oo = __builtin_fmaf(rpos.x, rpos.x, __builtin_fmaf(rpos.y, rpos.y, rpos.z * rpos.z));
    CHECK(same(t.ooBound, oo + ps.sphereBound), "case %d: ooBound", id);
    for (int k = 0; k < n; k += 2) {
        const float* q = sphq + 4 * k;
        for (int h = 0; h < 2; h++) {
            const float cx = q[0 + h], cy = q[2 + h], cz = q[4 + h], kk = q[6 + h];
            const float co = __builtin_fmaf(cx, rpos.x, __builtin_fmaf(cy, rpos.y, cz * rpos.z));
            const float ct = __builtin_fmaf(-2.0f, co, oo) + kk;
            const float* r = t.pair[k / 2];
            CHECK(same(r[0 + h], cx) && same(r[2 + h], cy) && same(r[4 + h], cz) && same(r[6 + h], ct), "case %d: pair record %d half %d", id, k / 2, h);
        }
    }
    for (int i = 0; i < n; i++) {
        const rt_f3 off = rpos - rt_v3(sph[4 * i + 0], sph[4 * i + 1], sph[4 * i + 2]);
        const float qc = rt_dot(off, off) - sph[4 * i + 3];
        CHECK(same(t.sph[i][0], off.x) && same(t.sph[i][1], off.y) && same(t.sph[i][2], off.z) && same(t.sph[i][3], qc), "case %d: sphere %d", id, i);
    }
    /* traverse_flat + tri_test, reading the laid-out triangle space as the kernel does */
    const unsigned char* triSpace = ps.lay.arena ? ps.lay.pairBuf.data() : ps.lay.triBuf.data();
    int k = 0;
    for (int m = 0; m < (int)ps.dmodels.size(); m++) {
        const DModel& M = ps.dmodels[m];
        const rt_f3 lpos = rt_v3(M.w2l[0] * rpos.x + M.w2l[1] * rpos.y + M.w2l[2] * rpos.z + M.w2l[3] * 1.0f,
                                 M.w2l[4] * rpos.x + M.w2l[5] * rpos.y + M.w2l[6] * rpos.z + M.w2l[7] * 1.0f,
                                 M.w2l[8] * rpos.x + M.w2l[9] * rpos.y + M.w2l[10] * rpos.z + M.w2l[11] * 1.0f);
        CHECK(same(t.lpos[m][0], lpos.x) && same(t.lpos[m][1], lpos.y) && same(t.lpos[m][2], lpos.z), "case %d: lpos of model %d", id, m);
        const uint32_t code = M.rootCode;
        uint32_t count = (code >> 24) & 0x7fu, start = code & RT_CODE_MAX_INLINE_START;
        if (count == 0) { count = ps.lay.bigLeaves[2 * start + 1]; start = ps.lay.bigLeaves[2 * start]; }
        CHECK((int)count == (int)(s.models.size() ? (m + 1 < (int)s.models.size() ? s.models[m + 1].triOffset : (int)s.tris.size()) - s.models[m].triOffset : 0),
              "case %d: model %d: root leaf holds %u triangles", id, m, count);
        for (uint32_t i = 0; i < count; i++, k++) {
            DTri q;
            memcpy(&q, triSpace + ((size_t)(M.triBase + (int)start + 3 * (int)i) << 4), sizeof(q));
            const rt_f3 A = rt_v3(q.ax, q.ay, q.az), face = rt_v3(q.fx, q.fy, q.fz);
            const rt_f3 vro = lpos - A;
            const float d = rt_dot(vro, face);
            CHECK(k < RT_PRIMARY_MAX_TRIS, "case %d: more triangles than the cap in a table that is on", id);
            if (k < RT_PRIMARY_MAX_TRIS)
                CHECK(same(t.tri[k][0], vro.x) && same(t.tri[k][1], vro.y) && same(t.tri[k][2], vro.z) && same(t.tri[k][3], d), "case %d: triangle %d (model %d)", id, k, m);
        }
    }
}

int main(int argc, char** argv)
{
    const unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1ull;
    const int cases = argc > 2 ? atoi(argv[2]) : 40;
    g_state = seed * 0x9e3779b97f4a7c15ull + 12345ull;
    int on = 0, made = 0;
    /* ---- random scenes within the caps: the table is on and exact.  Sphere counts cover 0, 1, odd (the pair's tail), 32 */
    static const int sphereCounts[] = {0, 1, 2, 3, 16, 17, 31, 32};
    for (int c = 0; c < cases; c++) {
        const int nSph = sphereCounts[c % 8];
        const int nModels = (int)(rnd() % (RT_PRIMARY_MAX_MODELS + 1));
        int per[RT_PRIMARY_MAX_MODELS] = {0, 0, 0, 0}, left = RT_PRIMARY_MAX_TRIS;
        for (int m = 0; m < nModels; m++) { per[m] = 1 + (int)(rnd() % 4); if (m == 0 && (c & 1)) per[m] = 2; left -= per[m]; }
        if (nModels && (c % 5) == 0) per[nModels - 1] += left; /* exactly at the triangle cap */
        const Scene s = make_scene(nSph, nModels, per, false);
        float cam[16];
        random_camera(cam);
        PreparedScene ps; PrimaryTris pt; PrimaryTable t;
        if (!build(s, cam, 0.0f, true, ps, pt, t)) continue;
        made++;
        CHECK(ps.flat, "case %d: leaf-root models make a FLAT scene", c);
        CHECK(t.on == 1, "case %d: table off for a scene within the caps (%d spheres, %d models)", c, nSph, nModels);
        if (t.on) { on++; verify(s, cam, ps, t, c); }
    }
    /* ---- the table is off */
    {
        const int per[RT_PRIMARY_MAX_MODELS + 1] = {2, 2, 2, 2, 2};
        float cam[16];
        random_camera(cam);
        auto off = [&](const char* what, const Scene& s, const float* cm, float defocus, bool sw) {
            PreparedScene ps; PrimaryTris pt; PrimaryTable t;
            if (build(s, cm, defocus, sw, ps, pt, t)) CHECK(t.on == 0, "table on: %s", what);
        };
        const Scene ok = make_scene(5, 2, per, false);
        { PreparedScene ps; PrimaryTris pt; PrimaryTable t; if (build(ok, cam, 0.0f, true, ps, pt, t)) { CHECK(t.on == 1, "control scene"); if (t.on) verify(ok, cam, ps, t, -1); } }
        off("defocus != 0", ok, cam, 100.0f, true);
        off("the run-time switch", ok, cam, 0.0f, false);
        for (int d = 0; d < 3; d++) { /* an origin component of -0 */
            float cz[16];
            memcpy(cz, cam, sizeof(cz));
            cz[12 + d] = -0.0f;
            for (int k = 0; k < 3; k++) cz[4 * k + d] = -fabsf(cz[4 * k + d]); /* (-x) * 0 = -0 in every term of the row */
            const rt_f3 o = primary_cam_origin(cz);
            CHECK(rt_f2u(d == 0 ? o.x : d == 1 ? o.y : o.z) == 0x80000000u, "the -0 camera of component %d is no -0", d);
            off("camera origin component -0", ok, cz, 0.0f, true);
        }
        {
            float cn[16];
            memcpy(cn, cam, sizeof(cn)); cn[13] = std::numeric_limits<float>::infinity();
            off("infinite camera", ok, cn, 0.0f, true);
            memcpy(cn, cam, sizeof(cn)); cn[5] = std::numeric_limits<float>::quiet_NaN();
            off("NaN camera", ok, cn, 0.0f, true);
        }
        off("33 spheres", make_scene(33, 1, per, false), cam, 0.0f, true);
        off("5 models", make_scene(3, 5, per, false), cam, 0.0f, true);
        { const int big[4] = {9, 8, 0, 0}; off("17 triangles", make_scene(3, 2, big, false), cam, 0.0f, true); }
        { const int big[4] = {17, 0, 0, 0}; off("17 triangles in one leaf", make_scene(0, 1, big, false), cam, 0.0f, true); }
        {
            const Scene inner = make_scene(3, 2, per, true);
            PreparedScene ps; PrimaryTris pt; PrimaryTable t;
            if (build(inner, cam, 0.0f, true, ps, pt, t)) { CHECK(!ps.flat, "an inner root makes the scene non-FLAT"); CHECK(t.on == 0, "table on: non-FLAT scene"); }
        }
        { /* a sphere so far away that its terms overflow: no agreed NaN bits, so off */
            Scene far = make_scene(2, 1, per, false);
            far.spheres[1].centre[0] = 3e38f; far.spheres[1].centre[1] = 3e38f;
            off("non-finite table entry", far, cam, 0.0f, true);
        }
    }
    if (failures) { printf("FAILED %d checks\n", failures); return 1; }
    printf("ok cases=%d on=%d\n", made, on);
    return 0;
}
