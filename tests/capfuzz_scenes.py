"""Seeded scenes WITHIN the caps of the FLAT trace kernel's three tables (ray-tracing_amd/csrc/rt_primary.h, rt_tile_cand.h), and the
text forms tests/tile_cand_driver.cpp and tests/tile_tri_driver.cpp read.  A plain helper module: tests/test_tile_fuzz.py runs the family
through the host drivers and checks the conditions on the family itself, tests/test_gpu_tile_fuzz.py renders it on the device.

The caps: at most 4 models, 16 root-leaf triangles and 32 spheres, no defocus, every root a leaf.  scene(pkg, seed) stays within all of
them by construction (bvhQuality = Disabled: a mesh is its root leaf); scene_over_a_cap(pkg, seed) is the same scene with exactly one of
them exceeded.  Everything is drawn from pkg.meshes._lcg, one stream each for the camera and settings, the spheres and the models: the
family's conditions are checked on the CPU, so the scenes must be the same wherever they are made, whatever numpy is installed there, and
pushing the spheres over their cap must leave the camera and the models alone.

What a seed decides by table (so that every listed value occurs within any 24 consecutive seeds, see tests/test_tile_fuzz.py) and what it
draws:  the field of view FOVS[seed % 5]; the sphere count SPHERE_COUNTS[seed % 7]; the models' triangle counts SPLITS[seed % 8]; a strip
partition when seed % 4 == 3; the camera inside or within 1 % of the surface of sphere 0 when seed % 3 == 0; everything else is drawn."""
import math

import numpy as np

SEEDS = tuple(range(1, 25))
# six seeds whose triangle table has a tile with an empty mask (tests/test_tile_fuzz.py checks that on the host)
EMPTY_TRI_MASK_SEEDS = (2, 3, 11, 13, 17, 18)
OVER_A_CAP_KINDS = ("33 spheres", "5 models", "17 triangles", "defocusStrength = 1e-30", "a root that is not a leaf")

FOVS = (5.0, 30.0, 60.0, 90.0, 140.0)
SPHERE_COUNTS = (0, 1, 2, 3, 17, 31, 32)
# triangles per model.  12 = cube(), 2 = quad(), 13 = cube() and one soup triangle in one mesh, everything else a soup mesh.
# (12, 2, 1, 1), (1, 1, 1, 13) and (4, 4, 4, 4) are at both caps; in them a skipped first or middle model makes traverse_flat's
# tk / pr jump by 12, 2 or 1.
SPLITS = ((), (2,), (12, 2, 1, 1), (1, 1, 1, 13), (7, 2, 7), (12,), (4, 4, 4, 4), (3, 12))
DIVERGE = (0.0, 1.5, 3.0, 50.0)
BOUNCES = (0, 1, 4, 9)


class _Draw:
    def __init__(self, pkg, seed):
        self.rnd = pkg.meshes._lcg(seed)
        for _ in range(4):   # (the first values of an LCG seeded with small numbers are close to each other)
            self.rnd()

    def uni(self, lo, hi):
        return lo + (hi - lo) * self.rnd()

    def pick(self, seq):
        return seq[min(int(self.rnd() * len(seq)), len(seq) - 1)]

    def vec(self, lo, hi):
        return np.array([self.uni(lo, hi) for _ in range(3)])


def _material(pkg, d, glass):
    M = pkg.manager.RayTracingMaterial
    col = lambda lo=0.05: tuple(d.uni(lo, 1.0) for _ in range(3)) + (1.0,)
    if glass:   # RC:355: no backface culling
        return M(flag=pkg.abi.MATERIAL_GLASS, ior=d.uni(1.0, 2.2), smoothness=d.uni(0.5, 1.0), specularProbability=d.uni(0.5, 1.0),
                 absorption=col(0.0), absorptionMultiplier=d.uni(0.0, 2.0), diffuseCol=col())
    return M(flag=d.pick((pkg.abi.MATERIAL_DEFAULT, pkg.abi.MATERIAL_DEFAULT, pkg.abi.MATERIAL_CHECKERED)), diffuseCol=col(), emissionCol=col(0.0),
             specularCol=col(0.3), emissionStrength=d.pick((0.0, 0.0, 0.0, 4.0)), smoothness=d.uni(0.0, 1.0), specularProbability=d.uni(0.0, 1.0))


class _View:
    """the camera as the raygen sees it: pixel (x, y) is aimed at pos + R (x / (W - 1) - 0.5) planeW + U (y / (H - 1) - 0.5) planeH + F focus"""

    def __init__(self, cam, focus, w, h):
        rot = cam.transform.rotation_matrix()
        self.pos = np.array(cam.transform.position)
        self.R, self.U, self.F = rot[:, 0], rot[:, 1], rot[:, 2]
        self.tanY = math.tan(math.radians(cam.fieldOfView) * 0.5)
        self.tanX = self.tanY * w / h
        self.w, self.h = w, h

    def through_pixel(self, x, y):
        v = self.F + self.R * ((x / (self.w - 1) - 0.5) * 2 * self.tanX) + self.U * ((y / (self.h - 1) - 0.5) * 2 * self.tanY)
        return v / np.linalg.norm(v)

    def in_front(self, d, t, spread=1.2):
        return self.pos + t * (self.F + self.R * (d.uni(-spread, spread) * self.tanX) + self.U * (d.uni(-spread, spread) * self.tanY))


def _radius(d):
    return 0.02 * (3.0 / 0.02) ** d.rnd()   # 0.02 ... 3, every decade as likely as another


def _spheres(pkg, d, seed, n, view):
    """sphere 0: the camera inside it or within 1 % of its surface (seed % 3 == 0); then, as far as the count goes and rotated by the seed
    where it is below 5: one directly behind the camera (a discriminant, negative roots), one centred on the ray through a tile corner
    (tangent to the cones of the four tiles around it), one anywhere and a second one coincident with it; the rest anywhere in and
    around the frustum"""
    S = pkg.manager.Sphere
    kinds = ["behind", "corner", "anywhere", "coincident"]
    if n < 5:
        kinds = kinds[(seed // 7) % 4:] + kinds[:(seed // 7) % 4]
    out = []
    for i in range(n):
        kind = kinds[i - 1] if 1 <= i <= 4 else "anywhere"
        if i == 0:
            kind = ("inside", "near")[(seed // 3) % 2] if seed % 3 == 0 else (kinds[0] if n < 5 else "anywhere")
        if kind == "coincident" and not out:
            kind = "anywhere"
        r = _radius(d)
        if kind == "inside":
            r = d.uni(0.5, 3.0)
            c = view.pos + d.vec(-0.3, 0.3) * r
        elif kind == "near":   # the camera 0.5 % of the radius outside or inside the surface
            r = d.uni(0.3, 3.0)
            v = d.vec(-1, 1) + view.F
            c = view.pos + v / np.linalg.norm(v) * (r * d.pick((0.995, 1.005)))
        elif kind == "behind":
            c = view.pos - view.F * (r + d.uni(0.1, 6.0))
        elif kind == "corner":
            r = d.uni(0.02, 0.3)
            tx, ty = 1 + int(d.rnd() * max((view.w - 1) // 8, 1)), 1 + int(d.rnd() * max((view.h - 1) // 8, 1))
            c = view.pos + view.through_pixel(8 * tx - 0.5, 8 * ty - 0.5) * d.uni(3.0, 12.0)
        elif kind == "coincident":
            c, r = np.array(out[-1].centre), out[-1].radius
        else:
            c = view.in_front(d, r + d.uni(1.0, 14.0))
        out.append(S(tuple(float(v) for v in c), float(r), _material(pkg, d, glass=(i + seed) % 3 == 0)))
    return out


def _soup(pkg, d, n, l2w, view, name):
    """n random triangles in the model's space; as far as n goes: one whose plane contains the camera, a degenerate one (C on AB) and a
    sliver (C a ten-thousandth beside AB)"""
    w2l = np.linalg.inv(l2w)
    cam_local = (w2l @ np.append(view.pos, 1.0))[:3]
    verts, norms = [], []
    for i in range(n):
        a = d.vec(-1, 1)
        b, c = a + d.vec(-1, 1), a + d.vec(-1, 1)
        if n >= 2 and i == 0:
            c = cam_local + (a - cam_local) * d.uni(-1.5, 1.5) + (b - cam_local) * d.uni(0.2, 1.5)
        elif n >= 3 and i == 1:
            c = a + (b - a) * d.uni(0.1, 0.9)
        elif n >= 4 and i == 2:
            c = a + (b - a) * d.uni(0.1, 0.9) + d.vec(-1e-4, 1e-4)
        nrm = np.cross(b - a, c - a)
        ln = np.linalg.norm(nrm)
        nrm = nrm / ln if ln > 1e-9 else np.array([0.0, 0.0, 1.0])
        verts += [a, b, c]
        norms += [nrm] * 3
    return pkg.meshes.Mesh(np.array(verts), np.array(norms), np.arange(3 * n), name)


def _join(pkg, a, b, name):
    return pkg.meshes.Mesh(np.concatenate([a.vertices, b.vertices]), np.concatenate([a.normals, b.normals]),
                           np.concatenate([a.triangles, b.triangles + len(a.vertices)]), name)


def _models(pkg, d, seed, split, view, big_mesh=None):
    """rotated, non-uniformly scaled models in and around the frustum; every third mirrored (one or three negative scales); the first quad
    of a scene, or else its first soup mesh, scaled 40 x 40 x 1 across the frustum and behind the camera; every third material glass"""
    T, Model = pkg.manager.Transform, pkg.manager.Model
    out, ground = [], False
    for i, n in enumerate(split):
        scale = d.vec(0.3, 2.5)
        pos = view.in_front(d, d.uni(2.0, 14.0))
        euler = tuple(d.uni(0, 360) for _ in range(3))
        if not ground and (n == 2 or (2 not in split and n not in (12, 13))):
            ground = True
            scale = np.array([40.0, 40.0, 1.0])
            pos = view.pos + np.array([d.uni(-2, 2), d.uni(-3.0, -0.5), d.uni(0, 6)])
            euler = (90 + d.uni(-12, 12), d.uni(0, 360), 0.0) if n == 2 else euler
        if (i + seed) % 3 == 1:
            scale = scale * (np.array([-1.0, -1.0, -1.0]) if (i + seed) % 2 else np.roll(np.array([-1.0, 1.0, 1.0]), i))
        tr = T(tuple(float(v) for v in pos), euler, tuple(float(v) for v in scale))
        if big_mesh is not None and i == 0:
            mesh = big_mesh
        elif n == 2:
            mesh = pkg.meshes.quad()
        elif n == 12:
            mesh = pkg.meshes.cube()
        elif n == 13:
            mesh = _join(pkg, pkg.meshes.cube(), _soup(pkg, d, 1, tr.localToWorldMatrix, view, "one"), f"CubeAndOne{seed}")
        else:
            mesh = _soup(pkg, d, n, tr.localToWorldMatrix, view, f"Soup{seed}_{i}")
        out.append(Model(mesh, _material(pkg, d, glass=(i + seed) % 3 == 0), tr))
    return out


def partition_of(seed):
    """(strip_rows, index, count) of the part a seed renders as, or None: every fourth seed is one part of a strip partition"""
    if seed % 4 != 3:
        return None
    count = 2 + (seed // 4) % 2
    return (8 if (seed // 8) % 2 else 16, (seed // 3) % count, count)


def _build(pkg, seed, n_spheres=None, split=None, defocus=0.0, big_mesh=None):
    d = _Draw(pkg, 4 * seed)
    T, Camera = pkg.manager.Transform, pkg.manager.Camera
    w, h = 9 + int(d.rnd() * 72), 9 + int(d.rnd() * 42)
    if d.rnd() < 0.2:   # mostly not multiples of 8
        w, h = (w + 7) // 8 * 8, (h + 7) // 8 * 8
    part = partition_of(seed)
    if part:   # (every part has rows)
        h = min(max(h, part[0] * (part[2] - 1) + 3), 50)
    roll = d.uni(-25, 25) if d.rnd() < 0.4 else 0.0
    cam = Camera(T(tuple(d.uni(-1, 1) + o for o in (0.0, 1.0, -5.0)), (d.uni(-20, 20), d.uni(-30, 30), roll)), fieldOfView=FOVS[seed % 5], aspect=w / h)
    focus = d.uni(0.5, 6.0)
    settings = dict(maxBounceCount=d.pick(BOUNCES), numRaysPerPixel=1 + int(d.rnd() * 3), divergeStrength=d.pick(DIVERGE), defocusStrength=defocus,
                    focusDistance=focus, useSky=d.rnd() < 0.6, sunFocus=d.uni(100, 900), sunIntensity=d.uni(1, 20), accumulate=True,
                    bvhQuality=pkg.abi.BVH_QUALITY_HIGH if big_mesh is not None else pkg.abi.BVH_QUALITY_DISABLED)
    view = _View(cam, focus, w, h)
    spheres = _spheres(pkg, _Draw(pkg, 4 * seed + 1), seed, SPHERE_COUNTS[seed % 7] if n_spheres is None else n_spheres, view)
    models = _models(pkg, _Draw(pkg, 4 * seed + 2), seed, SPLITS[seed % 8] if split is None else split, view, big_mesh)
    sc = pkg.scenes.SceneDescription(f"capfuzz{seed}", w, h, 3, settings, cam, models, spheres)
    return sc, int(_Draw(pkg, 4 * seed + 3).rnd() * 2**31)


def scene(pkg, seed):
    """-> (SceneDescription, render seed): within every cap"""
    return _build(pkg, seed)


def scene_over_a_cap(pkg, seed):
    """scene(pkg, seed) with OVER_A_CAP_KINDS[seed % 5] changed and nothing else: the camera, the settings and the other half of the
    geometry are the in-cap scene's"""
    kind = seed % 5
    if kind == 0:
        return _build(pkg, seed, n_spheres=33)
    if kind == 1:
        return _build(pkg, seed, split=(2, 1, 3, 1, 2))
    if kind == 2:
        return _build(pkg, seed, split=(12, 2, 3))
    if kind == 3:
        return _build(pkg, seed, defocus=1e-30)
    return _build(pkg, seed, split=(80, 2), big_mesh=pkg.meshes.icosphere(1))   # 80 triangles: the builder splits the root


def triangle_counts(sc):
    return tuple(m.Mesh.triangle_count for m in sc.models)


# ---- the host drivers' text forms --------------------------------------------------------------------------------------------------

class _NoTracer:
    """make_manager wants a tracer; params() never calls it"""

    def __getattr__(self, name):
        raise AssertionError(f"the tracer is not to be called ({name})")


def _camera_lines(mgr, w, h, part):
    p = mgr.params()
    assert p.defocusStrength == 0.0
    return [f"{w} {h} {part[0]} {part[1]} {part[2]} {p.divergeStrength!r}",
            " ".join(repr(float(v)) for v in p.camLocalToWorld),
            " ".join(repr(float(v)) for v in p.viewParams)]


def write_sphere_scene(pkg, api, sc, path, w=None, h=None, part=(8, 0, 1)):
    """the camera block and spheres of a scene as the manager hands them to the library, in tests/tile_cand_driver.cpp's text form"""
    mgr = sc.make_manager(_NoTracer(), api, w, h)
    w, h = mgr.screenSize
    lines = _camera_lines(mgr, w, h, part) + [str(len(mgr.spheres))]
    for s in mgr.spheres:
        lines.append(" ".join(repr(float(np.float32(v))) for v in (*s.centre, s.radius)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def write_triangle_scene(pkg, api, sc, path, w=None, h=None, part=(8, 0, 1)):
    """the camera block and the models' root leaves of a scene as the manager hands them to the library, in tests/tile_tri_driver.cpp's
    text form: per model the worldToLocal rows as pack_model lays them out, cull (RC:355), and the root leaf's triangles in the builder's order"""
    mgr = sc.make_manager(_NoTracer(), api, w, h)
    w, h = mgr.screenSize
    data = mgr.CreateAllMeshData(mgr.models)
    info, tris, nodes = data["meshInfo"], data["triangles"], data["nodes"]
    lines = _camera_lines(mgr, w, h, part) + [str(len(mgr.models))]
    for i, model in enumerate(mgr.models):
        m = info[i]["worldToLocal"]
        root = nodes[int(info[i]["nodeOffset"])]
        n = int(root["triangleCount"])
        assert n > 0, "the driver's scenes are FLAT: every model's root is a leaf"
        lines.append(" ".join(repr(float(m[c * 4 + r])) for r in range(3) for c in range(4)))
        lines.append(f"{int(model.material.flag != pkg.abi.MATERIAL_GLASS)} {n}")
        first = int(info[i]["triOffset"]) + int(root["startIndex"])
        for t in tris[first:first + n]:
            lines.append(" ".join(repr(float(v)) for v in (*t["posA"], *t["posB"], *t["posC"])))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def sphere_scene_file(pkg, api, d, cfg, w, h, part=(8, 0, 1)):
    """a config's sphere file in directory d (tests/test_tile_cand.py)"""
    return write_sphere_scene(pkg, api, pkg.scenes.get(cfg), str(d / f"config{cfg}_{w}x{h}_{part[1]}of{part[2]}.txt"), w, h, part)


def triangle_scene_file(pkg, api, d, cfg, w, h, part=(8, 0, 1), change=None, tag=""):
    """a config's triangle file in directory d, the scene first passed through change(sc) (tests/test_tile_tri.py)"""
    sc = pkg.scenes.get(cfg)
    if change:
        change(sc)
    return write_triangle_scene(pkg, api, sc, str(d / f"config{cfg}{tag}_{w}x{h}_{part[1]}of{part[2]}.txt"), w, h, part)


WALK_SEEDS = (2, 4, 6, 12, 13, 18, 22)        # scenes with spheres and models
OTHER_IN_CAP = (19, 11, 3, 23, 20, 6, 12)     # what upload_scene replaces them with
STEPS = 10


def _walk(pkg, seed):
    """the walk of a seed as plain data, so that the library's manager and the oracle's take the very same steps.  Four of the six plain
    kinds (which two are left out rotates with the seed) and the six that come once per walk, shuffled; the second in-cap upload comes
    two steps after the over-the-cap one and defocus goes on early enough to go off again two steps later."""
    d = _Draw(pkg, 7919 * seed + 1)
    plain = ["sphere", "model", "camera", "fov", "diverge", "reset"]
    idx = WALK_SEEDS.index(seed)
    for k in sorted({idx % 6, (idx + 3) % 6}, reverse=True):
        del plain[k]
    kinds = plain + ["defocus", "resize_same_tiles", "resize", "upload_in_cap", "upload_over_a_cap", "upload_in_cap_again"]
    assert len(kinds) == STEPS
    for i in range(len(kinds) - 1, 0, -1):
        j = int(d.rnd() * (i + 1))
        kinds[i], kinds[j] = kinds[j], kinds[i]
    if kinds.index("defocus") > STEPS - 3:
        kinds.remove("defocus")
        kinds.insert(int(d.rnd() * (STEPS - 2)), "defocus")
    kinds.remove("upload_in_cap_again")   # over a cap for two steps, not for most of the walk: the steps are there to change a table's key
    kinds.insert(min(kinds.index("upload_over_a_cap") + 2, len(kinds)), "upload_in_cap_again")
    if kinds.index("defocus") > STEPS - 3:   # (pushed back by the insertion)
        kinds.remove("defocus")
        kinds.insert(0, "defocus")
    steps = []
    for i, kind in enumerate(kinds):
        steps.append(dict(kind=kind, u=[d.rnd() for _ in range(12)], k=2 + int(d.rnd() * 4), over=idx % 3, other=OTHER_IN_CAP[idx] if kind == "upload_in_cap" else seed))
    return steps
