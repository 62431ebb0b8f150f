"""What tests/test_gpu_nee.py and tests/test_nee.py compare include/rt_nee.h's calls with: the estimator of the header restated path by
path in Python, and the light table restated in numpy.

  * every path segment and every shadow ray goes through rt_query_closest (existing, bit-pinned code: tests/test_gpu_query.py holds it
    to the oracle), all paths of a batch at once per bounce; each such ray is logged (Estimator.segment_log, .shadow_log), so that a
    test can say from the rays themselves what its batch covered;
  * the draws and the shader's functions come from the oracle: random_value, random_direction, material_colour, reflectance, refract,
    environment_light; sqrt, divide, reciprocal, rsqrt, exp, sin and cos from oracle_math_eval (rt_math.h's, which
    tests/test_gpu_math.py pins the device against); everything else is numpy float32, one rounding per operation, in the header's order;
  * the table is float64 Python arithmetic rounded to float32, written from the header text and independently of
    ray-tracing_amd/csrc/rt_light_table.h.

Test infrastructure: nothing here is imported by the product."""
import ctypes as C
import math

import numpy as np

F = np.float32
F3 = C.c_float * 3
GLASS = 2
PI = F(3.1415926)
PI2 = F(2) * F(3.1415926)
EPS = F(0.001)


# ---------------------------------------------------------------- amendment 1: the table
def _emitter(mat):
    le = (mat["emissionCol"][:3] * mat["emissionStrength"]).astype(F)
    ok = int(mat["flag"]) != GLASS and bool(np.isfinite(le).all()) and bool((le > 0).any())
    return ok, le


def _to_world(m, p):
    return np.array([m[r] * p[0] + m[4 + r] * p[1] + m[8 + r] * p[2] + m[12 + r] * F(1) for r in range(3)], dtype=F)


def light_table(abi, models, triangles, spheres):
    """{entries (abi.LIGHT_ENTRY_DTYPE), cdf (float32), in_table (bool per object), n_sphere_entries, n_triangle_entries}"""
    models = np.zeros(0, dtype=abi.model_dtype) if models is None else np.asarray(models, dtype=abi.model_dtype)
    triangles = np.zeros(0, dtype=abi.triangle_dtype) if triangles is None else np.asarray(triangles, dtype=abi.triangle_dtype)
    spheres = np.zeros(0, dtype=abi.sphere_dtype) if spheres is None else np.asarray(spheres, dtype=abi.sphere_dtype)
    entries, weights = [], []
    in_table = np.zeros(len(spheres) + len(models), dtype=bool)
    n_sphere = n_tri = 0
    with np.errstate(all="ignore"):
        for s in range(len(spheres)):
            ok, le = _emitter(spheres[s]["material"])
            r = spheres[s]["radius"]
            if not ok or not (r > 0) or not np.isfinite(r):
                continue
            e = np.zeros((), dtype=abi.LIGHT_ENTRY_DTYPE)
            e["a"], e["size"], e["object"], e["triangle"], e["emission"] = spheres[s]["centre"], r * r, s, -1, le
            entries.append(e)
            weights.append((4.0 * math.pi * (float(r) * float(r))) * float(le.max()))
            in_table[s] = True
            n_sphere += 1
        offsets = sorted(int(o) for o in models["triOffset"])
        for m in range(len(models)):
            ok, le = _emitter(models[m]["material"])
            if not ok:
                continue
            l2w = models[m]["localToWorld"]
            a, b, c, d, e_, f, g, h, i = (float(l2w[k]) for k in (0, 4, 8, 1, 5, 9, 2, 6, 10))
            mirrored = a * (e_ * i - f * h) - b * (d * i - f * g) + c * (d * h - e_ * g) < 0.0
            start = int(models[m]["triOffset"])
            end = min([o for o in offsets if o > start], default=len(triangles))
            for k in range(start, end):
                t = triangles[k]
                A = _to_world(l2w, t["posA"])
                B = _to_world(l2w, t["posC"] if mirrored else t["posB"])
                Cc = _to_world(l2w, t["posB"] if mirrored else t["posC"])
                E1 = [float(B[q]) - float(A[q]) for q in range(3)]
                E2 = [float(Cc[q]) - float(A[q]) for q in range(3)]
                X = [E1[1] * E2[2] - E1[2] * E2[1], E1[2] * E2[0] - E1[0] * E2[2], E1[0] * E2[1] - E1[1] * E2[0]]
                L = math.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2])
                S = F(0.5 * L)
                if not (S > 0) or not np.isfinite(S):
                    continue
                ng = np.array([X[q] / L for q in range(3)]).astype(F)
                if not np.isfinite(ng).all():
                    continue
                e = np.zeros((), dtype=abi.LIGHT_ENTRY_DTYPE)
                e["a"], e["size"], e["e1"], e["e2"], e["ng"] = A, S, B - A, Cc - A, ng
                e["object"], e["triangle"], e["emission"] = len(spheres) + m, k, le
                entries.append(e)
                weights.append(float(S) * float(le.max()))
                in_table[len(spheres) + m] = True
                n_tri += 1
        n = len(entries)
        out = np.zeros(n, dtype=abi.LIGHT_ENTRY_DTYPE)
        cdf = np.zeros(n, dtype=F)
        total = 0.0
        for w in weights:
            total += w
        run = 0.0
        for k in range(n):
            out[k] = entries[k]
            run += weights[k]
            cdf[k] = F(run / total)
            out[k]["prob"] = F(weights[k] / total)
        if n:
            cdf[n - 1] = F(1)
    return {"entries": out, "cdf": cdf, "in_table": in_table, "n_sphere_entries": n_sphere, "n_triangle_entries": n_tri}


def pick(cdf, u):
    """The smallest i with u < cdf[i]; the last entry when there is none."""
    return min(int(np.searchsorted(cdf, F(u), side="right")), len(cdf) - 1)


def _material(abi, emission=(0, 0, 0), strength=0.0, flag=0):
    m = np.zeros((), dtype=abi.material_dtype)
    m["diffuseCol"], m["specularCol"] = (0.5, 0.5, 0.5, 1), (1, 1, 1, 1)
    m["emissionCol"], m["emissionStrength"], m["flag"], m["specularProbability"], m["ior"] = tuple(emission) + (1,), strength, flag, 1.0, 1.0
    return m


def table_test_scene(abi):
    """Arrays (no BVH needed) with every rule of amendment 1 in them: spheres that are emitters and spheres excluded for each reason;
    a mesh of two triangles used by an emissive model, a dark one and a mirrored emissive one; a second mesh with a degenerate, a
    proper and a point triangle under a rotated, unevenly scaled transform; a glass model."""
    spheres = np.zeros(8, dtype=abi.sphere_dtype)
    rows = [((0, 5, 0), 1.25, (1, 0.9, 0.8), 8.0, 0), ((3, 0, 0), 1.0, (1, 1, 1), 2.0, GLASS), ((6, 0, 0), 1.0, (1, np.nan, 1), 2.0, 0),
            ((9, 0, 0), 1.0, (1, 1, 1), 0.0, 1), ((12, 0, 0), 0.0, (1, 1, 1), 2.0, 0), ((15, 1, 0), 0.3, (0.2, 0.7, 0.1), 3.0, 1),
            ((18, 0, 0), 1.0, (1, 1, 1), -2.0, 0), ((21, 0, 2), 0.07, (-1, 0, 0.5), 11.0, 0)]
    for s, (c, r, col, strength, flag) in zip(spheres, rows):
        s["centre"], s["radius"], s["material"] = c, r, _material(abi, col, strength, flag)
    tris = np.zeros(5, dtype=abi.triangle_dtype)
    corners = [((0, 0, 0), (1, 0, 0), (1, 1, 0)), ((0, 0, 0), (1, 1, 0), (0, 1, 0)), ((0, 0, 0), (1, 0, 0), (2, 0, 0)),
               ((0.1, 0.2, 0.3), (2.2, 0.1, -0.4), (0.3, 1.9, 0.7)), ((1, 1, 1), (1, 1, 1), (1, 1, 1))]
    for t, (a, b, c) in zip(tris, corners):
        t["posA"], t["posB"], t["posC"] = a, b, c
        t["normA"] = t["normB"] = t["normC"] = (0, 0, 1)
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])  # orthonormal
    mats = [np.diag([2.0, 3.0, 1.0]), np.eye(3), np.diag([-1.0, 1.0, 1.0]), rot @ np.diag([0.7, 1.3, 2.1]), np.eye(3)]
    rows = [(0, mats[0], (10, 0, 5), (1, 1, 1), 4.0, 0), (0, mats[1], (0, 0, 0), (1, 1, 1), 0.0, 0), (0, mats[2], (0, 0, 1), (0, 2, 0), 1.0, 0),
            (2, mats[3], (0.5, -3, 0.25), (1, 0.5, 0.25), 1.5, 0), (2, mats[4], (0, 0, 0), (1, 0, 0), 1.0, GLASS)]
    models = np.zeros(5, dtype=abi.model_dtype)
    for m, (off, lin, pos, col, strength, flag) in zip(models, rows):
        l2w = np.eye(4)
        l2w[:3, :3], l2w[:3, 3] = lin, pos
        m["triOffset"], m["material"] = off, _material(abi, col, strength, flag)
        m["localToWorld"], m["worldToLocal"] = l2w.T.reshape(16).astype(F), np.linalg.inv(l2w).T.reshape(16).astype(F)
    return models, tris, spheres


# ---------------------------------------------------------------- the estimator
def _dot(a, b):
    p = a * b
    return (p[0] + p[1]) + p[2]


def _max(a, b):  # rt_max
    return a if (a > b or b != b) else b


class Estimator:
    """rt_nee_trace of a batch, from the header text.  `tracer` holds the scene
    (its rt_query_closest walks the segments); models / triangles / spheres are the arrays it was given; p the RtParams."""

    def __init__(self, pkg, orc, tracer, models, triangles, spheres, p):
        assert b"RT_MATH_IEEE" not in orc.version()
        self.abi, self.orc, self.tr, self.p = pkg.abi, orc, tracer, p
        self.n_spheres = len(spheres)
        self.spheres = spheres
        self.materials = np.ascontiguousarray(np.concatenate([spheres["material"], models["material"]]))
        self.table = light_table(pkg.abi, models, triangles, spheres)
        self.shadow_rays = self.samples = self.unshadowed = self.suppressed = self.inside = self.triangle_samples = 0  # what a batch covered
        # every ray trace() walked, in the order it walked them (appended to by every call; the records do not depend on them):
        self.segment_log = []  # (ray index, bounce, origin, direction) of every path segment
        self.shadow_log = []   # (ray index, bounce, origin, direction, wanted object, wanted triangle, unshadowed) of every shadow ray
        self._x = np.zeros(1, dtype=F)
        self._y = np.zeros(1, dtype=F)
        self._o = np.zeros(1, dtype=F)

    def ev(self, op, x, y=0.0):
        self._x[0], self._y[0] = x, y
        self.orc.math_eval(op, self._x.ctypes.data, self._y.ctypes.data, self._o.ctypes.data, 1)
        return F(self._o[0])

    def normalize(self, v):
        return (v * self.ev(8, _dot(v, v))).astype(F)

    def rand(self, st):
        return F(self.orc.random_value(C.byref(st)))

    def sample(self, st, x, n):
        """Amendment 2's draws and arithmetic: None, or (omega, g, Le, object, triangle)."""
        t = self.table
        u0, u1, u2 = self.rand(st), self.rand(st), self.rand(st)
        e = t["entries"][pick(t["cdf"], u0)]
        prob, obj, tri, le = e["prob"], int(e["object"]), int(e["triangle"]), e["emission"].astype(F)
        self.samples += 1
        if tri < 0:
            w = e["a"] - x
            d2, r2 = _dot(w, w), e["size"]
            if not d2 > r2:
                self.inside += 1
                return None
            s2 = self.ev(6, r2, d2)
            cmax = self.ev(4, F(1) - s2)
            q = self.ev(6, s2, F(1) + cmax)
            ct = F(1) - u1 * q
            st_ = self.ev(4, _max(F(0), F(1) - ct * ct))
            ang = PI2 * u2
            sn, cs = self.ev(2, ang), self.ev(3, ang)
            z = self.normalize(w)
            sg = np.copysign(F(1), z[2])
            a = -self.ev(9, sg + z[2])
            b = z[0] * z[1] * a
            b1 = np.array([F(1) + sg * z[0] * z[0] * a, sg * b, -sg * z[0]], dtype=F)
            b2 = np.array([b, sg + z[1] * z[1] * a, -z[1]], dtype=F)
            omega = (b1 * (st_ * cs) + b2 * (st_ * sn) + z * ct).astype(F)
            cn = _dot(n, omega)
            if not cn > 0:
                return None
            g = self.ev(6, cn * F(2) * q, prob)
            return omega, g, le, obj, tri
        self.triangle_samples += 1
        fold = u1 + u2 > F(1)
        v1, v2 = (F(1) - u1, F(1) - u2) if fold else (u1, u2)
        y = (e["a"] + e["e1"] * v1 + e["e2"] * v2).astype(F)
        v = y - x
        d2 = _dot(v, v)
        omega = self.normalize(v)
        cl = _dot(e["ng"], -omega)
        cn = _dot(n, omega)
        if not (cl > 0 and cn > 0):
            return None
        g = self.ev(6, cn * cl * e["size"], PI * d2 * prob)
        return omega, g, le, obj, tri

    def trace(self, rays):
        abi, orc, p = self.abi, self.orc, self.p
        rays = np.ascontiguousarray(rays, dtype=abi.PATHRAY_DTYPE).reshape(-1)
        n = len(rays)
        out = np.zeros(n, dtype=abi.RADIANCE_DTYPE)
        out["rng"] = rays["rng"]
        if p.maxBounceCount < 0 or n == 0:
            return out
        pos, dirs = rays["origin"].copy(), rays["dir"].copy()
        T, L = np.ones((n, 3), dtype=F), np.zeros((n, 3), dtype=F)
        rng = [C.c_uint32(int(s)) for s in rays["rng"]]
        bounce = np.zeros(n, dtype=np.int64)
        prev = np.zeros(n, dtype=bool)
        active = np.arange(n)
        o3 = F3()
        with np.errstate(all="ignore"):
            while len(active):
                hits = self.tr.query_closest(abi.make_rays(pos[active], dirs[active]))
                ended, shadows = [], []
                for j, i in enumerate(active):
                    h, st = hits[j], rng[i]
                    vertex = int(bounce[i])  # the path's segment, and the vertex at its end, counted from 0
                    self.segment_log.append((int(i), vertex, pos[i].copy(), dirs[i].copy()))
                    if h["object"] < 0:
                        if p.useSky:
                            orc.environment_light(C.byref(p), F3(*dirs[i]), o3)
                            L[i] = L[i] + T[i] * np.array(o3[:], dtype=F)
                        ended.append(i)
                        continue
                    obj = int(h["object"])
                    mat = self.materials[obj]
                    normal, hpos, rdir = h["normal"].astype(F), h["pos"].astype(F), dirs[i].copy()
                    backface = bool(h["hit"] & 0x100)
                    sample = False
                    if int(mat["flag"]) == GLASS:
                        if backface:
                            e = ((-h["dst"]) * mat["absorption"][:3]) * mat["absorptionStrength"]
                            T[i] = T[i] * np.array([self.ev(1, e[0]), self.ev(1, e[1]), self.ev(1, e[2])], dtype=F)
                        ior_a, ior_b = (float(mat["ior"]), 1.0) if backface else (1.0, float(mat["ior"]))
                        orc.refract(F3(*rdir), F3(*normal), ior_a, ior_b, o3)
                        refract_dir = np.array(o3[:], dtype=F)
                        weight = F(orc.reflectance(F3(*rdir), F3(*normal), ior_a, ior_b))
                        orc.random_direction(C.byref(st), o3)
                        diffuse = self.normalize(normal + np.array(o3[:], dtype=F))
                        reflect_dir = rdir - (F(2) * _dot(rdir, normal)) * normal
                        if self.rand(st) <= weight:
                            a, b, t = diffuse, reflect_dir, mat["specularProbability"]
                        else:
                            a, b, t = -diffuse, refract_dir, mat["smoothness"]
                        ndir = self.normalize(a + (b - a) * t)
                        d = _dot(normal, ndir)
                        npos = hpos + (EPS * normal) * F(int(d > 0) - int(d < 0))
                    else:
                        specular = bool(mat["specularProbability"] >= self.rand(st))
                        orc.random_direction(C.byref(st), o3)
                        diffuse = self.normalize(normal + np.array(o3[:], dtype=F))
                        reflect_dir = rdir - (F(2) * _dot(rdir, normal)) * normal
                        t = mat["smoothness"] * (F(1) if specular else F(0))
                        emitted = mat["emissionCol"][:3] * mat["emissionStrength"]
                        counted = prev[i] and self.table["in_table"][obj] and not (obj < self.n_spheres and backface)
                        if counted:
                            self.suppressed += 1
                        else:
                            L[i] = L[i] + emitted * T[i]
                        orc.material_colour(self.materials[obj:obj + 1].ctypes.data, F3(*hpos), F3(*normal), int(specular), o3)
                        T[i] = T[i] * np.array(o3[:], dtype=F)
                        sample = len(self.table["cdf"]) > 0 and bool(t == 0)
                        ndir = self.normalize(diffuse + (reflect_dir - diffuse) * t)
                        npos = hpos + normal * EPS
                    pos[i], dirs[i] = npos, ndir
                    prev[i] = sample
                    if sample:
                        s = self.sample(st, pos[i].copy(), normal)
                        if s is not None:
                            omega, g, le, want_obj, want_tri = s
                            shadows.append((i, pos[i].copy(), omega, ((T[i] * le) * g).astype(F), want_obj, want_tri, vertex))
                    pr = _max(T[i][0], _max(T[i][1], T[i][2]))
                    if self.rand(st) >= pr:
                        ended.append(i)
                    else:
                        T[i] = T[i] * self.ev(9, pr)
                        bounce[i] += 1
                        if bounce[i] > p.maxBounceCount:
                            ended.append(i)
                if shadows:
                    sh = self.tr.query_closest(abi.make_rays(np.array([s[1] for s in shadows]), np.array([s[2] for s in shadows])))
                    self.shadow_rays += len(shadows)
                    for (i, spos, sdir, light, want_obj, want_tri, vertex), h in zip(shadows, sh):
                        seen = int(h["object"]) == want_obj and (want_tri < 0 or int(h["triangle"]) == want_tri)
                        if seen:
                            L[i] = L[i] + light
                            self.unshadowed += 1
                        self.shadow_log.append((int(i), vertex, spos, sdir, want_obj, want_tri, seen))
                for i in ended:
                    out["rgb"][i] = F(0) + L[i]
                    out["rng"][i] = rng[i].value
                gone = set(ended)
                active = np.array([i for i in active if i not in gone], dtype=np.int64)
        return out


# ---------------------------------------------------------------- the scenes the GPU tests build
def _desc(pkg, name, models, spheres, cam_pos, cam_euler=(0, 0, 0), sky=False, bounces=4):
    cam = pkg.Camera(pkg.Transform(cam_pos, cam_euler), fieldOfView=60.0)
    settings = dict(maxBounceCount=bounces, numRaysPerPixel=1, divergeStrength=0.5, useSky=sky, accumulate=True, bvhQuality=1)
    return pkg.scenes.SceneDescription(name, 64, 36, 1, settings, cam, models, spheres)


def _floor(pkg, size=12.0, rho=0.8):
    """A diffuse quad in the plane y = 0 that faces up (the Quad's front normal is local -z)."""
    M, T = pkg.RayTracingMaterial, pkg.Transform
    return pkg.Model(pkg.meshes.quad(), M(diffuseCol=(rho, rho, rho, 1), specularProbability=0.0), T((0, 0, 0), (90, 0, 0), (size, size, 1)), "Floor")


def build_scene(pkg, name):
    """The scenes of tests/test_gpu_nee.py that no other test has, by name."""
    M, T, S, Model = pkg.RayTracingMaterial, pkg.Transform, pkg.Sphere, pkg.Model
    if name == "nee_flat":  # three spheres, two of them emissive, and a two-triangle quad light: every root a leaf
        spheres = [S((0, 1, 0), 1.0, M(diffuseCol=(0.8, 0.7, 0.6, 1), specularProbability=0.0)),
                   S((-2.5, 2.5, 0.5), 0.4, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.6, 0.3, 1), emissionStrength=9.0)),
                   S((2.2, 0.6, -0.8), 0.6, M(diffuseCol=(0.3, 0.3, 0.3, 1), emissionCol=(0.2, 0.5, 1, 1), emissionStrength=3.0, specularProbability=0.3, smoothness=0.7))]
        light = Model(pkg.meshes.quad(), M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 1, 0.9, 1), emissionStrength=12.0), T((0.5, 3.5, 0), (-90, 0, 0), (1.5, 1.0, 1)), "QuadLight")
        return _desc(pkg, name, [_floor(pkg), light], spheres, (0, 1.5, -6), sky=True)
    if name == "nee_mirrored":  # a quad light whose transform has a negative determinant, facing the floor below it
        m = np.array([[1.5, 0, 0, 0.3], [0, 0, 1, 2.5], [0, 1.2, 0, 0.2], [0, 0, 0, 1]], dtype=np.float64)  # local -z (the front) -> world -y
        assert np.linalg.det(m[:3, :3]) < 0
        light = Model(pkg.meshes.quad(), M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.8, 0.6, 1), emissionStrength=10.0), pkg.MatrixTransform(m), "MirroredLight")
        spheres = [S((0.3, 1.0, 0.2), 0.6, M(diffuseCol=(0.7, 0.3, 0.3, 1), specularProbability=0.0))]  # under the light: it shadows the floor below
        return _desc(pkg, name, [_floor(pkg), light], spheres, (0, 1.2, -5))
    if name == "nee_glass":  # a glass sphere between the light and the floor
        spheres = [S((0, 4.0, 0), 0.5, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 1, 1, 1), emissionStrength=10.0)),
                   S((0, 1.6, 0), 0.9, M(flag=GLASS, ior=1.5, smoothness=1.0, specularProbability=1.0, absorption=(0.2, 0.1, 0.4, 1), absorptionMultiplier=0.5)),
                   S((1.8, 0.5, 0.5), 0.5, M(diffuseCol=(0.3, 0.6, 0.8, 1), specularProbability=0.0))]
        return _desc(pkg, name, [_floor(pkg)], spheres, (0, 1.5, -5.5))
    if name == "nee_inside":  # the camera and everything it sees lie inside an emissive sphere; a second emitter is inside as well
        spheres = [S((0, 0, 0), 6.0, M(diffuseCol=(0.5, 0.5, 0.5, 1), emissionCol=(0.3, 0.4, 0.5, 1), emissionStrength=1.0, specularProbability=0.0)),
                   S((0, 0, 1.5), 1.0, M(diffuseCol=(0.8, 0.8, 0.8, 1), specularProbability=0.0)),
                   S((1.8, 1.6, 0.5), 0.3, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.7, 0.2, 1), emissionStrength=20.0))]
        return _desc(pkg, name, [], spheres, (0, 0, -3))
    if name == "nee_mirrors":  # every surface a perfect mirror: no diffuse vertex anywhere
        mirror = dict(smoothness=1.0, specularProbability=1.0)
        spheres = [S((0, 1, 0), 1.0, M(diffuseCol=(0.9, 0.9, 0.9, 1), specularCol=(0.9, 0.8, 0.7, 1), **mirror)),
                   S((0, 4.0, 0), 0.7, M(diffuseCol=(0, 0, 0, 1), specularCol=(0.5, 0.5, 0.5, 1), emissionCol=(1, 1, 1, 1), emissionStrength=6.0, **mirror)),
                   S((2.1, 0.7, 0.3), 0.7, M(specularCol=(0.6, 0.9, 0.6, 1), **mirror))]
        floor = _floor(pkg)
        floor.material = M(diffuseCol=(0.8, 0.8, 0.8, 1), specularCol=(0.8, 0.8, 0.8, 1), **mirror)
        return _desc(pkg, name, [floor], spheres, (0, 1.5, -6), sky=True)
    if name == "nee_instances":
        # one mesh of 320 triangles (a tree with inner nodes, its triangles reordered by the builder) under three models: an emissive
        # instance low over the floor, an emissive instance above and beside it under a mirroring, unevenly scaled, rotated transform —
        # the lower one hides part of it from the floor — and a dark one; a small emissive sphere; a floor and a ceiling.  The emitters
        # are diffuse too: paths go on from them, and sample their own far side.
        ball = pkg.meshes.icosphere(2, radius=1.0)
        lin = T((0, 0, 0), (25, 40, 10)).rotation_matrix() @ np.diag([-0.9, 0.55, 0.75])
        assert np.linalg.det(lin) < 0
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = lin, (0.2, 2.4, 0.4)
        ceiling = Model(pkg.meshes.quad(), M(diffuseCol=(0.7, 0.7, 0.7, 1), specularProbability=0.0), T((0, 5.5, 0), (-90, 0, 0), (40, 40, 1)), "Ceiling")  # (faces down:
        # paths that leave the floor go on, and its vertices see the instances from above)
        models = [_floor(pkg, 40.0), ceiling,
                  Model(ball, M(diffuseCol=(0.6, 0.5, 0.4, 1), emissionCol=(1, 0.8, 0.5, 1), emissionStrength=4.0, specularProbability=0.0), T((-0.2, 1.1, 0.3), (0, 0, 0), 0.65), "BallLight"),
                  Model(ball, M(diffuseCol=(0.4, 0.5, 0.6, 1), emissionCol=(0.4, 0.6, 1, 1), emissionStrength=6.0, specularProbability=0.0), pkg.MatrixTransform(m), "MirroredBallLight"),
                  Model(ball, M(diffuseCol=(0.7, 0.7, 0.3, 1), specularProbability=0.0), T((2.1, 0.75, -0.6), (0, 30, 0), (0.7, 0.75, 0.6)), "DarkBall")]
        spheres = [S((-2.3, 0.45, -0.8), 0.25, M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.9, 0.7, 1), emissionStrength=15.0))]
        return _desc(pkg, name, models, spheres, (0, 3.2, -6), (22, 0, 0))  # looking down: nearly every camera ray starts a path that samples
    raise KeyError(name)
