"""What the tests of the ray queries (tests/test_gpu_query.py) share with the tests of the passes that trace caller-made rays: the scenes as
rt_upload_scene takes them, the ray mix, the oracle's records (computed once per scene and process, shared, never written) and the comparisons."""
import ctypes as C
import os

import numpy as np

from gpu_support import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
F3 = C.c_float * 3
SCENES = ["config2_flat", "config3_bvh", "crowded70_many", "glass_balls"]


def crowded_identity_scene(pkg, n_models=70, n_spheres=5, seed=7):
    """More models than the 64-bit root-filter mask holds (the MANY variant: two-level filter, candidate masks extended into LDS).  Models 0
    and 1 — a cube, and a ball that pokes through its faces — stand at the origin untransformed (rule 2's identity case); every fourth
    model and the first sphere are glass."""
    rng = np.random.default_rng(seed)
    M, T = pkg.RayTracingMaterial, pkg.Transform
    meshes = [pkg.meshes.cube(), pkg.meshes.icosphere(1, radius=0.7), pkg.meshes.rounded_cube(3), pkg.meshes.quad()]
    models = []
    for i in range(n_models):
        tf = T() if i < 2 else T(tuple(rng.uniform(-4, 4, 3) + [0, 1.5, 4]), tuple(rng.uniform(0, 360, 3)), float(rng.uniform(0.3, 0.9)))
        models.append(pkg.Model(meshes[i % 4], M(flag=int(i % 4 == 3) * 2, diffuseCol=tuple(rng.uniform(0.2, 1, 3)) + (1,), ior=1.4), tf))
    spheres = [pkg.Sphere(tuple(rng.uniform(-4, 4, 3) + [0, 1.5, 4]), float(rng.uniform(0.3, 0.8)),
                          M(flag=int(i % 5 == 0) * 2, diffuseCol=tuple(rng.uniform(0.2, 1, 3)) + (1,), ior=1.5))
               for i in range(n_spheres)]
    cam = pkg.Camera(T((0, 1.5, -6), (0, 0, 0)), fieldOfView=55.0)
    settings = dict(maxBounceCount=2, numRaysPerPixel=1, divergeStrength=0.5, useSky=True, accumulate=True, bvhQuality=1)
    return pkg.scenes.SceneDescription("crowded70", 64, 36, 1, settings, cam, models, spheres)


def scene_of(pkg, name):
    if name == "config2_flat":
        return pkg.scenes.get(2)
    if name == "config3_bvh":
        return pkg.scenes.get(3)
    if name == "crowded70_many":
        return crowded_identity_scene(pkg)
    if name == "glass_balls":
        return pkg.sceneio.load_scene(os.path.join(ROOT, "ray-tracing_amd", "scenes_data", "glass_balls.json"))
    raise KeyError(name)


class Scene:
    """A scene's arrays, as rt_upload_scene takes them, and what the checks need of them.  upload() gives a tracer the scene and nothing
    else: no rt_resize, no rt_set_params."""

    def __init__(self, pkg, lib, name):
        self.name = name
        self.desc = scene_of(pkg, name)
        self.mgr = self.desc.make_manager(None, lib, 64, 36)
        data = self.mgr.CreateAllMeshData(self.mgr.models)
        self.models, self.triangles, self.nodes = data["meshInfo"], data["triangles"], data["nodes"]
        self.spheres = self.mgr._pack_spheres()
        self.n_spheres = len(self.spheres)
        self.materials = np.concatenate([self.spheres["material"], self.models["material"]])
        self.tri_count = np.array([m.Mesh.triangle_count for m in self.mgr.models], dtype=np.int64)
        # world-space points of everything: the scene's bounds, and origins inside objects
        pts, self.centres = [], []
        for m in self.mgr.models:
            l2w = np.asarray(m.transform.localToWorldMatrix, dtype=np.float64)
            v = np.asarray(m.Mesh.vertices, dtype=np.float64).reshape(-1, 3) @ l2w[:3, :3].T + l2w[:3, 3]
            pts.append(v)
            self.centres.append(v.mean(axis=0))
        for s in self.mgr.spheres:
            c = np.array(s.centre)
            pts += [c[None] - s.radius, c[None] + s.radius]
            self.centres.append(c)
        pts = np.concatenate(pts)
        # (a ground plane hundreds of units wide would make every ray start far from everything else: the bounds are those of the
        # middle of the scene, the 5th to 95th percentile of its points per axis)
        self.lo, self.hi = np.percentile(pts, 5, axis=0), np.percentile(pts, 95, axis=0)
        self.centres = np.array(self.centres)

    def upload(self, tracer):
        tracer.upload_scene(self.models, self.triangles, self.nodes, self.spheres)
        return tracer


def make_rays(sc, n=2000, seed=11):
    """The batch of a scene, from a fixed seed: (n, 3) float32 origins and directions.
      33 %  origins on a sphere around the bounds, aimed at random points inside them (normalised)
      32 %  origins on that sphere, looking away from the scene (a random direction of the outward hemisphere): most miss
      12 %  origins at (near) the centres of spheres and meshes, random directions: back faces
      10 %  unnormalised directions, |dir| = 0.25 and 7
      10 %  axis-parallel directions: two components exactly 0
       3 %  degenerates: a zero direction, a NaN component, an infinite origin component"""
    rng = np.random.default_rng(seed)
    centre, half = (sc.lo + sc.hi) / 2, (sc.hi - sc.lo) / 2
    radius = 1.6 * float(np.linalg.norm(half)) + 0.5

    def on_sphere(k):
        v = rng.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def inside(k):
        return centre + rng.uniform(-1, 1, (k, 3)) * half

    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    counts = [int(n * f) for f in (0.33, 0.32, 0.12, 0.10, 0.10)]
    o, d = [], []
    a = centre + radius * on_sphere(counts[0])
    o.append(a), d.append(unit(inside(counts[0]) - a))
    out = on_sphere(counts[1])
    away = on_sphere(counts[1])
    away *= np.where((away * out).sum(axis=1, keepdims=True) < 0, -1.0, 1.0)
    o.append(centre + radius * out), d.append(away)
    a = sc.centres[rng.integers(0, len(sc.centres), counts[2])] + rng.uniform(-0.02, 0.02, (counts[2], 3))
    o.append(a), d.append(on_sphere(counts[2]))
    a = centre + radius * on_sphere(counts[3])
    scale = np.where(np.arange(counts[3]) % 2 == 0, 0.25, 7.0)[:, None]
    o.append(a), d.append(unit(inside(counts[3]) - a) * scale)
    axis = rng.integers(0, 3, counts[4])
    sign = rng.choice([-1.0, 1.0], counts[4])
    a = inside(counts[4])
    dd = np.zeros((counts[4], 3))
    dd[np.arange(counts[4]), axis] = sign
    a[np.arange(counts[4]), axis] = centre[axis] - sign * radius  # outside the bounds, looking in along the axis
    o.append(a), d.append(dd)
    k = n - sum(counts)
    a, dd = inside(k), on_sphere(k)
    for i in range(k):
        if i % 3 == 0:
            dd[i] = 0.0
        elif i % 3 == 1:
            dd[i, i % 2] = np.nan
        else:
            a[i, (i // 3) % 3] = np.inf if i % 2 else -np.inf
    o.append(a), d.append(dd)
    return np.concatenate(o).astype(F), np.concatenate(d).astype(F)


def oracle_hits(orc, ot, origins, dirs):
    """(n, 10) float32: oracle_ray_collision per ray — didHit, isBackface, dst, normal, pos, material flag."""
    out = np.zeros((len(origins), 10), dtype=F)
    out10 = (C.c_float * 10)()
    for i in range(len(origins)):
        orc.ray_collision(ot.h, F3(*origins[i]), F3(*dirs[i]), out10)
        out[i] = out10[:]
    return out


_CACHE = {}


def case(pkg, api, orc, name):
    """Scene, rays and the oracle's records of a scene: computed once, shared by the tests, never written."""
    if name not in _CACHE:
        sc = Scene(pkg, api, name)
        origins, dirs = make_rays(sc)
        ot = orc.create_tracer(1)
        try:
            sc.upload(ot)
            want = oracle_hits(orc, ot, origins, dirs)
        finally:
            ot.close()
        for a in (origins, dirs, want):
            a.setflags(write=False)
        _CACHE[name] = (sc, origins, dirs, want)
    return _CACHE[name]


def assert_same_records(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for f in got.dtype.names:
        a, b = bits(got[f]).reshape(len(got), -1), bits(want[f]).reshape(len(want), -1)
        bad = np.argwhere((a != b).any(axis=1)).ravel()
        assert not len(bad), f"{what}: field {f}: {len(bad)} rays differ; first is ray {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def records_from_oracle(pkg, sc, want10, objects, triangles):
    """The RtRayHit records the oracle's ten values stand for.  oracle_ray_collision names neither object nor triangle: the GPU's own
    answers are taken over and checked apart (rule 2)."""
    abi = pkg.abi
    rec = np.zeros(len(want10), dtype=abi.RAYHIT_DTYPE)
    hit = want10[:, 0] != 0
    rec["dst"] = want10[:, 2]
    rec["normal"][hit] = want10[hit, 3:6]
    rec["pos"][hit] = want10[hit, 6:9]
    cls = np.where(want10[:, 9] == abi.MATERIAL_GLASS, 2, 1).astype(np.uint32)
    rec["hit"] = np.where(hit, cls | np.where(want10[:, 1] != 0, abi.AOV_HIT_BACKFACE, 0).astype(np.uint32), 0)
    rec["object"] = np.where(hit, objects, -1)
    rec["triangle"] = np.where(hit, triangles, -1)
    return rec


def snapshot(tr):
    c = tr.counters()
    c.pop("gpuMs")
    return dict(frame=tr.frame(), counters=c, accumulated=tr.read_accumulated().tobytes(), last=tr.read_frame().tobytes(),
                tiles=tr.adaptive_tiles().tobytes(), tile_error=tr.adaptive_tile_error().tobytes(), moments=tr.read_moments().tobytes())
