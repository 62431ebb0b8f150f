"""What the tests of the AOV pass (tests/test_gpu_aov.py) share with the tests of the passes built on it: the scenes, a tracer set up through
the manager, camera ray 0 restated in fp32 from the oracle's functions, the records the oracle gives for those rays, and the comparisons."""
import ctypes as C
import os

import numpy as np

from fuzz_scenes import crowded_overflow_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
F3 = C.c_float * 3


def emitter_scene(pkg, defocus):
    """10 opaque models (four meshes; two with identity transforms) and 3 spheres, each an emitter of strength 1 with a colour of its
    own made of small dyadic values; no sky, no bounce, one ray per pixel: a rendered frame shows, per pixel, the first hit's emission."""
    M, T = pkg.RayTracingMaterial, pkg.Transform
    meshes = [pkg.meshes.cube(), pkg.meshes.icosphere(1, radius=0.7), pkg.meshes.quad(), pkg.meshes.rounded_cube(3)]
    palette = [((1 + k % 4) / 4.0, (1 + (k // 4) % 4) / 8.0, (1 + k % 3) / 2.0) for k in range(13)]
    assert len(set(palette)) == 13
    rng = np.random.default_rng(3)
    models = []
    for i in range(10):  # models 0 and 1 (a cube, and a ball that pokes through its faces) stand at the origin untransformed
        tf = T() if i in (0, 1) else T(tuple(rng.uniform(-2.5, 2.5, 3) * [1, 0.6, 0.6] + [0, 0.3, 2.5]), tuple(rng.uniform(0, 360, 3)), float(rng.uniform(0.6, 1.1)))
        models.append(pkg.Model(meshes[i % 4], M(diffuseCol=(0.5, 0.5, 0.5, 1), emissionCol=palette[3 + i] + (1,), emissionStrength=1.0), tf))
    spheres = [pkg.Sphere(c, r, M(diffuseCol=(0.3, 0.3, 0.3, 1), emissionCol=palette[i] + (1,), emissionStrength=1.0))
               for i, (c, r) in enumerate((((-1.6, 1.2, 1.0), 0.5), ((1.7, -0.6, 0.5), 0.4), ((0.3, -1.4, 3.0), 0.9)))]
    cam = pkg.Camera(T((0, 0.3, -3.2), (0, 0, 0)), fieldOfView=60.0)
    settings = dict(maxBounceCount=0, numRaysPerPixel=1, divergeStrength=0.7, defocusStrength=defocus, focusDistance=3.0, useSky=False,
                    accumulate=True, bvhQuality=1)
    return pkg.scenes.SceneDescription("emitters", 64, 36, 1, settings, cam, models, spheres), palette


def scene_of(pkg, spec):
    if spec == "crowded70":  # more than 64 models: the two-level filter and the candidate masks in LDS (MANY)
        return crowded_overflow_scene(pkg, 70, 5)
    if spec in ("emitters", "emitters_dof"):
        return emitter_scene(pkg, 60.0 if spec == "emitters_dof" else 0.0)[0]
    if spec == "glass_balls_file":
        return pkg.sceneio.load_scene(os.path.join(ROOT, "ray-tracing_amd", "scenes_data", "glass_balls.json"))
    cfg, kw = spec
    return pkg.scenes.get(cfg, **kw)


class Setup:
    """A tracer driven through the manager up to (not including) the first frame, with what was uploaded kept for the checks."""

    def __init__(self, pkg, lib, tracer, spec, w, h, tweak=None, seed=1):
        self.tr = tracer
        self.scene = {}
        upload = tracer.upload_scene

        def keep(models, triangles, nodes, spheres=None):
            self.scene = dict(models=np.array(models), triangles=np.array(triangles), spheres=np.array(spheres))
            return upload(models, triangles, nodes, spheres)
        tracer.upload_scene = keep
        self.mgr = scene_of(pkg, spec).make_manager(tracer, lib, w, h)
        for k, v in (tweak or {}).items():
            setattr(self.mgr, k, v)
        self.mgr.OnEnable(renderSeed=seed)
        self.w, self.h = w, h
        self.n_spheres = len(self.scene["spheres"])
        self.materials = np.concatenate([self.scene["spheres"]["material"], self.scene["models"]["material"]])
        # a model's triangle range: the triangles of its mesh, from its triOffset
        self.tri_count = np.array([m.Mesh.triangle_count for m in self.mgr.models], dtype=np.int64)

    def params(self, frame):
        p = self.mgr.params()
        p.frame = frame
        return p


def oracle_eval(orc, op, x, y=None):
    x = np.ascontiguousarray(x, dtype=F)
    y = np.ascontiguousarray(np.zeros_like(x) if y is None else np.broadcast_to(np.asarray(y, dtype=F), x.shape), dtype=F)
    out = np.zeros_like(x)
    orc.math_eval(op, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size)
    return out


def camera_rays(orc, p, w, h, frame, rows=None):
    """Origin and direction of camera ray 0 of frame `frame` for every pixel of the global rows `rows` (default: all) of a w x h image:
    (len(rows), w, 3) float32 each.  One fp32 rounding per operation, in the reference's order."""
    ieee = b"RT_MATH_IEEE" in orc.version()
    rows = np.arange(h) if rows is None else np.asarray(rows)
    with np.errstate(all="ignore"):
        # RCC:15: id.xy / (Resolution - 1.0)
        uvx = oracle_eval(orc, 6, np.arange(w, dtype=np.uint32).astype(F), F(w) - F(1))
        uvy = oracle_eval(orc, 6, rows.astype(np.uint32).astype(F), F(h) - F(1))
        U, V = np.broadcast_to(uvx[None, :], (len(rows), w)), np.broadcast_to(uvy[:, None], (len(rows), w))
        # RC:550-552 (a NaN uv — a one-pixel-wide or -high image — converts to 0, as the device's conversion does)
        pcx = np.where(np.isnan(U), F(0), U * F(w)).astype(np.uint64)
        pcy = np.where(np.isnan(V), F(0), V * F(h)).astype(np.uint64)
        rng0 = ((pcy * w + pcx) + np.uint64(frame) * np.uint64(719393) + np.uint64(p.renderSeed & 0xffffffff)) & np.uint64(0xffffffff)
        m = np.array(list(p.camLocalToWorld), dtype=F)
        vp = np.array(list(p.viewParams), dtype=F)

        def mul_point(x, y, z):  # mul(M, float4(v, 1)).xyz, summed left to right
            return [m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * F(1) for r in range(3)]
        focus = mul_point((U - F(0.5)) * vp[0], (V - F(0.5)) * vp[1], np.full(U.shape, F(1) * vp[2], dtype=F))
        zero = np.zeros(U.shape, dtype=F)
        cam_origin = mul_point(zero, zero, zero)
        right, up = m[0:3], m[4:7]
        # RC:565-572: the two draws, per pixel, from the oracle's own generator
        dj = np.zeros(U.shape + (2,), dtype=F)
        jj = np.zeros(U.shape + (2,), dtype=F)
        out2 = (C.c_float * 2)()
        for idx in np.ndindex(U.shape):
            st = C.c_uint32(int(rng0[idx]))
            orc.random_point_in_circle(C.byref(st), out2)
            dj[idx] = (out2[0], out2[1])
            orc.random_point_in_circle(C.byref(st), out2)
            jj[idx] = (out2[0], out2[1])
        dx = oracle_eval(orc, 6, dj[..., 0] * F(p.defocusStrength), F(w))
        dy = oracle_eval(orc, 6, dj[..., 1] * F(p.defocusStrength), F(w))
        jx = oracle_eval(orc, 6, jj[..., 0] * F(p.divergeStrength), F(w))
        jy = oracle_eval(orc, 6, jj[..., 1] * F(p.divergeStrength), F(w))
        origin = [cam_origin[k] + right[k] * dx + up[k] * dy for k in range(3)]
        jfp = [focus[k] + right[k] * jx + up[k] * jy for k in range(3)]
        d = [jfp[k] - origin[k] for k in range(3)]
        dot = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if ieee:
            n = oracle_eval(orc, 4, dot)
            direction = [oracle_eval(orc, 6, d[k], n) for k in range(3)]
        else:
            r = oracle_eval(orc, 8, dot)  # rt_normalize = v * rt_rsqrt(dot(v, v))
            direction = [d[k] * r for k in range(3)]
    return np.stack(origin, axis=-1).astype(F), np.stack(direction, axis=-1).astype(F)


def oracle_records(pkg, orc, ot, su, p, origins, dirs, objects):
    """The records the oracle's functions give for these rays.  oracle_ray_collision does not name the object: `objects` (the AOV's own
    answer) selects the material, whose flag must then be the one the oracle's hit carries; object and triangle are checked apart."""
    abi = pkg.abi
    want = np.zeros(origins.shape[:2], dtype=abi.AOV_DTYPE)
    want["object"] = -1
    want["triangle"] = -1
    out10 = (C.c_float * 10)()
    out3 = F3()
    for idx in np.ndindex(want.shape):
        o, d = F3(*origins[idx]), F3(*dirs[idx])
        orc.ray_collision(ot.h, o, d, out10)
        r = np.array(out10[:], dtype=F)
        w = want[idx]
        w["dst"] = r[2]
        if r[0] != 0:
            obj = int(objects[idx])
            assert 0 <= obj < len(su.materials), (idx, obj)
            mat = su.materials[obj:obj + 1].copy()
            assert int(mat["flag"][0]) == int(r[9]), ("material flag of the AOV's object != the oracle's hit", idx, obj, int(mat["flag"][0]), float(r[9]))
            w["normal"], w["pos"] = r[3:6], r[6:9]
            w["hit"] = (2 if int(r[9]) == abi.MATERIAL_GLASS else 1) | (abi.AOV_HIT_BACKFACE if r[1] != 0 else 0)
            orc.material_colour(mat.ctypes.data, F3(*r[6:9]), F3(*r[3:6]), 0, out3)
            w["albedo"] = out3[:]
            w["emission"] = mat["emissionCol"][0][:3] * mat["emissionStrength"][0]  # RC:530: one fp32 multiply each
            w["object"] = obj
            # HitInfo.pos as the oracle formed it: origin + dir * dst
            pos = origins[idx] + dirs[idx] * r[2]
            assert pos.view(np.uint32).tolist() == r[6:9].view(np.uint32).tolist(), (idx, pos, r[6:9])
        elif p.useSky:
            orc.environment_light(C.byref(p), d, out3)
            w["albedo"] = out3[:]
    return want


FLOAT_FIELDS = ("dst", "normal", "pos", "albedo", "emission")


def assert_records_equal(got, want, what, fields=None):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for f in fields or got.dtype.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        a, b = (a.view(np.uint32), b.view(np.uint32)) if f in FLOAT_FIELDS else (a, b)
        bad = np.argwhere(a.reshape(got.shape + (-1,)) != b.reshape(got.shape + (-1,)))
        if len(bad):
            y, x = bad[0][:2]
            raise AssertionError(f"{what}: field {f}: {len(set(map(tuple, bad[:, :2])))} pixels differ; first at row {y}, column {x}: got {got[y, x]}, want {want[y, x]}")


def check_triangles(orc, su, aov, origins, dirs):
    """Rule 6.  Returns how many pixels were checked against oracle_ray_triangle."""
    models, tris = su.scene["models"], su.scene["triangles"]
    identity = np.eye(4, dtype=F).T.reshape(16)
    is_model = aov["object"] >= su.n_spheres
    assert ((aov["triangle"] >= 0) == is_model).all(), "triangle is -1 exactly where no model was hit"
    out6 = (C.c_float * 6)()
    checked = 0
    for idx in np.argwhere(is_model):
        idx = tuple(idx)
        mi = int(aov["object"][idx]) - su.n_spheres
        t = int(aov["triangle"][idx])
        off = int(models["triOffset"][mi])
        assert off <= t < off + int(su.tri_count[mi]), (idx, mi, t, off, int(su.tri_count[mi]))
        if np.array_equal(models["localToWorld"][mi], identity) and np.array_equal(models["worldToLocal"][mi], identity):
            cull = int(models["material"]["flag"][mi]) != 2  # RC:355
            orc.ray_triangle(F3(*origins[idx]), F3(*dirs[idx]), tris[t:t + 1].ctypes.data, int(cull), out6)
            assert out6[0] != 0, (idx, "the reported triangle is not hit by the pixel's ray")
            got = np.array([aov["dst"][idx]], dtype=F).view(np.uint32)[0]
            assert np.array([out6[2]], dtype=F).view(np.uint32)[0] == got, (idx, out6[2], aov["dst"][idx])
            checked += 1
    return checked
