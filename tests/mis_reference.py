"""What tests/test_gpu_mis.py and tests/test_mis.py compare include/rt_mis.h's call with: the estimator of the header restated path by
path in Python, and the reverse map restated in numpy.  As tests/nee_reference.py, which this module imports for the table, the pick
rule, the scenes and Estimator's helpers:

  * every path segment and every shadow ray goes through rt_query_closest, all paths of a batch at once per bounce;
  * the draws and the shader's functions come from the oracle, sqrt / divide / reciprocal / rsqrt / exp / sin / cos from
    oracle_math_eval; everything else is numpy float32, one rounding per operation, in the header's order;
  * per path it logs each light sample (sample_log: g, sphere or triangle, seen or not), each emission behind a sampled vertex
    (emission_log: wb and the rule that made it what it is; emission_hits: the object and triangle that was hit) and each last-vertex
    sample that was skipped (skipped_log).

Test infrastructure: nothing here is imported by the product."""
import ctypes as C

import numpy as np

import nee_reference as nr

F = np.float32
F3 = nr.F3
PI, PI2, EPS, GLASS = nr.PI, nr.PI2, nr.EPS, nr.GLASS
NO_ENTRY = 0xFFFFFFFF
_dot, _max = nr._dot, nr._max

# emission_log rules: why wb is what it is
WEIGHTED = "weighted"      # wb = pbPrev / (pbPrev + pl')
NO_ENTRY_RULE = "no entry"  # the hit object / triangle has no entry: in full
INSIDE = "inside"          # a sphere hit from inside: in full
NOT_LOBE = "cn' <= 0"      # the lobe could not have taken the direction: wb = 1
NOT_CONE = "d2 <= r2"      # the sampler takes no sample from inside the sphere: wb = 1
BACK = "cl <= 0"           # the sampler rejects the triangle's back: wb = 1
NAN = "nan"                # pl' not computable: wb = 1


def light_map(table, n_objects):
    """entry(object, triangle) of include/rt_mis.h as a dict {(object, triangle): index}; a missing key is NONE."""
    out = {}
    for i, e in enumerate(table["entries"]):
        assert 0 <= int(e["object"]) < n_objects
        out[(int(e["object"]), int(e["triangle"]))] = i
    return out


def map_arrays(abi, models, triangles, spheres):
    """The map in rt_debug_light_map's layout, restated: (objects, triangle words)."""
    table = nr.light_table(abi, models, triangles, spheres)
    models = np.zeros(0, dtype=abi.model_dtype) if models is None else np.asarray(models, dtype=abi.model_dtype)
    n_sph = 0 if spheres is None else len(spheres)
    n_tris = 0 if triangles is None else len(triangles)
    entry = light_map(table, n_sph + len(models))
    objects = np.full(n_sph + len(models), NO_ENTRY, dtype=np.uint32)
    words = []
    offsets = sorted(int(o) for o in models["triOffset"])
    for s in range(n_sph):
        objects[s] = entry.get((s, -1), NO_ENTRY)
    for m in range(len(models)):
        o = n_sph + m
        if not table["in_table"][o]:
            continue
        start = int(models[m]["triOffset"])
        end = min([x for x in offsets if x > start], default=n_tris)
        objects[o] = len(words)
        words += [entry.get((o, k), NO_ENTRY) for k in range(start, end)]
    return objects, np.array(words, dtype=np.uint32), table


class Estimator(nr.Estimator):
    """rt_mis_trace of a batch, from the header text."""

    def __init__(self, pkg, orc, tracer, models, triangles, spheres, p):
        super().__init__(pkg, orc, tracer, models, triangles, spheres, p)
        self.entry = light_map(self.table, len(spheres) + len(models))
        self.sample_log = []    # (ray, vertex, g, "sphere" | "triangle", seen) of every sample that reached its shadow walk
        self.emission_log = []  # (ray, vertex, wb, rule, "sphere" | "triangle") of every opaque hit behind a vertex that took a sample
        self.emission_hits = []  # (object, triangle) of the hit of every row of emission_log, in its order
        self.skipped_log = []   # (ray, vertex) of every diffuse vertex that took no sample because it was the path's last
        self.plain_emission_log = []  # (ray, vertex) of every opaque hit on an emitter whose previous vertex took no sample

    def balance(self, pa, pb, otherwise):
        w = self.ev(6, pa, pa + pb)
        return w if (w >= 0 and w <= 1) else F(otherwise)

    def sample(self, st, x, n):
        """The light sample: None, or (omega, g, Le, object, triangle)."""
        t = self.table
        u0, u1, u2 = self.rand(st), self.rand(st), self.rand(st)
        e = t["entries"][nr.pick(t["cdf"], u0)]
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
            g = self.balance(self.ev(6, cn, PI), self.ev(6, prob, PI2 * q), 0)
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
        g = self.balance(self.ev(6, cn, PI), self.ev(6, prob * d2, cl * e["size"]), 0)
        return omega, g, le, obj, tri

    def emission_weight(self, obj, tri, backface, cn_prev, x, rdir, hpos):
        """(wb, rule) for an opaque hit behind a vertex that took a sample."""
        sphere = obj < self.n_spheres
        if sphere and backface:
            return F(1), INSIDE
        i = self.entry.get((obj, -1 if sphere else tri))
        if i is None:
            return F(1), NO_ENTRY_RULE
        if not cn_prev > 0:
            return F(1), NOT_LOBE
        pb = self.ev(6, cn_prev, PI)
        e = self.table["entries"][i]
        prob = e["prob"]
        if sphere:
            w = e["a"] - x
            d2, r2 = _dot(w, w), e["size"]
            if not d2 > r2:
                return F(1), NOT_CONE
            s2 = self.ev(6, r2, d2)
            cmax = self.ev(4, F(1) - s2)
            q = self.ev(6, s2, F(1) + cmax)
            pl = self.ev(6, prob, PI2 * q)
        else:
            v = hpos - x
            d2 = _dot(v, v)
            cl = _dot(e["ng"], -rdir)
            if not cl > 0:
                return F(1), BACK
            pl = self.ev(6, prob * d2, cl * e["size"])
        w = self.ev(6, pb, pb + pl)
        if not (w >= 0 and w <= 1):
            return F(1), NAN
        return w, WEIGHTED

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
        cn_prev = np.zeros(n, dtype=F)
        active = np.arange(n)
        o3 = F3()
        with np.errstate(all="ignore"):
            while len(active):
                hits = self.tr.query_closest(abi.make_rays(pos[active], dirs[active]))
                ended, shadows = [], []
                for j, i in enumerate(active):
                    h, st = hits[j], rng[i]
                    vertex = int(bounce[i])
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
                        if prev[i]:
                            wb, rule = self.emission_weight(obj, int(h["triangle"]), backface, cn_prev[i], pos[i].copy(), rdir, hpos)
                            self.emission_log.append((int(i), vertex, float(wb), rule, "sphere" if obj < self.n_spheres else "triangle"))
                            self.emission_hits.append((obj, int(h["triangle"])))
                            L[i] = L[i] + (emitted * T[i]) * wb
                        else:
                            if self.table["in_table"][obj]:
                                self.plain_emission_log.append((int(i), vertex))
                            L[i] = L[i] + emitted * T[i]
                        orc.material_colour(self.materials[obj:obj + 1].ctypes.data, F3(*hpos), F3(*normal), int(specular), o3)
                        T[i] = T[i] * np.array(o3[:], dtype=F)
                        diffuse_vertex = len(self.table["cdf"]) > 0 and bool(t == 0)
                        sample = diffuse_vertex and vertex < p.maxBounceCount
                        if diffuse_vertex and not sample:
                            self.skipped_log.append((int(i), vertex))
                        ndir = self.normalize(diffuse + (reflect_dir - diffuse) * t)
                        npos = hpos + normal * EPS
                    pos[i], dirs[i] = npos, ndir
                    prev[i] = sample
                    if sample:
                        cn_prev[i] = _dot(normal, ndir)
                        s = self.sample(st, pos[i].copy(), normal)
                        if s is not None:
                            omega, g, le, want_obj, want_tri = s
                            shadows.append((i, pos[i].copy(), omega, ((T[i] * le) * g).astype(F), want_obj, want_tri, vertex, float(g)))
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
                    for (i, spos, sdir, light, want_obj, want_tri, vertex, g), h in zip(shadows, sh):
                        seen = int(h["object"]) == want_obj and (want_tri < 0 or int(h["triangle"]) == want_tri)
                        if seen:
                            L[i] = L[i] + light
                            self.unshadowed += 1
                        self.shadow_log.append((int(i), vertex, spos, sdir, want_obj, want_tri, seen))
                        self.sample_log.append((int(i), vertex, g, "sphere" if want_tri < 0 else "triangle", seen))
                for i in ended:
                    out["rgb"][i] = F(0) + L[i]
                    out["rng"][i] = rng[i].value
                gone = set(ended)
                active = np.array([i for i in active if i not in gone], dtype=np.int64)
        return out


# One row per rule constant above: the case (scene, maxBounceCount as in tests/test_gpu_mis.py's case()) whose emission_log must hold the rule,
# or None and why no table the library builds reaches it.  A rule marked unreachable must not be logged by ANY case: rules_allowed() is
# called by every MIS test that runs the reference (test_gpu_mis.py, test_gpu_deep_trees.py, test_gpu_many_models.py and
# test_gpu_hazards.py: four modules), so a change that makes one reachable is noticed where it happens.
RULE_TABLE = [
    (WEIGHTED, "sphere", ("nee_flat", None), ""),
    (WEIGHTED, "triangle", ("nee_flat", None), ""),
    (NO_ENTRY_RULE, None, ("config3_bvh", None), ""),
    (INSIDE, "sphere", ("nee_inside", None), ""),
    (BACK, "triangle", "mis_back_light", "reached only through a model record whose worldToLocal contradicts its localToWorld (back_light_case): an opaque model is always "
                                             "culled from behind, so no consistent scene hits a table triangle with cl <= 0"),
    (NOT_CONE, None, None, "needs a FRONT-face hit of a sphere from a segment origin inside it (d2 <= r2): a ray that starts inside a sphere leaves it through a back face"),
    (NOT_LOBE, None, None, "needs dot(n, normalize(n + RandomDirection)) <= 0 at a vertex that sampled: RandomDirection is a unit vector, so n + it lies in n's closed half space, "
                              "and the sum is 0 (a NaN direction, which hits nothing) only for the one draw -n"),
    (NAN, None, None, "needs prob * d2 and cl * S both 0 or both inf, or pb + pl' not finite: the table's area rule keeps S finite and > 0 and prob in (0, 1], cl is in (0, 1], and the "
                         "surface offset keeps d2 > 0"),
]
UNREACHABLE = {rule for (rule, _, where, _) in RULE_TABLE if where is None}


def rules_allowed(est, what):
    """no emission of this reference run was given its weight by a rule RULE_TABLE marks unreachable -> {rule: count}"""
    seen = {r: sum(1 for e in est.emission_log if e[3] == r) for r in sorted({e[3] for e in est.emission_log})}
    assert not set(seen) & UNREACHABLE, f"{what}: the reference logged {seen}; RULE_TABLE marks {sorted(set(seen) & UNREACHABLE)} unreachable"
    return seen
