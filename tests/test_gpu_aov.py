"""rt_render_aov / rt_render_aov_to_device (include/rt_aov.h) on the GPU: what camera ray 0 of a frame hits first, per pixel.
Every comparison is == on the bit patterns (uint32 views: NaN and -0 count), every pixel, every field.

  4. anchor without restated ray maths: in a scene of emitters (emissionStrength 1, distinct dyadic colours), no sky, no bounce, one
     ray per pixel, the oracle's rendered frame N IS the emission of what camera ray 0 hit (RC:485-538, 530-531 with a transmittance
     of exactly 1) — so aov.emission == the oracle's frame, and aov.object names that palette entry;
  5. every field against the oracle's functions: the test restates RCC:15 + RC:550-576 in fp32, one rounding per operation, with the
     draws from oracle_next_random / oracle_random_point_in_circle and the divide / normalise from oracle_math_eval, and feeds each
     ray to oracle_ray_collision, oracle_material_colour and oracle_environment_light; the restated rays are held by 4 and by
     HIP rt_debug_intersect on them == the AOV records;
  6. `triangle`: inside its model's range, and for identity-transform models oracle_ray_triangle on it returns the record's dst;
  7. hit class == rt_render_cost's firstHit;
  8. the same records under every device layout, strip partition, for 1 x N and N x 1 images, and through the device variant into a
     torch tensor;
  9. no visible state change;  10. errors, and the pass's own watchdog word (RT_TRAV_LIMIT, the hook tests/test_gpu_watchdog.py uses)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from flush_table import held_at

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
F3 = C.c_float * 3


class DevBuf:
    """Device memory through the HIP runtime the library already loaded (torch would bring a second runtime into this process: the
    torch test below runs in a child)."""

    def __init__(self, nbytes, fill=0):
        self.hip = C.CDLL("libamdhip64.so")
        self.nbytes = nbytes
        self.p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(nbytes)) == 0
        assert self.hip.hipMemset(self.p, fill, C.c_size_t(nbytes)) == 0 and self.hip.hipDeviceSynchronize() == 0

    @property
    def ptr(self):
        return self.p.value

    def records(self, pkg, h, w):
        out = np.zeros((h, w), dtype=pkg.abi.AOV_DTYPE)
        assert out.nbytes == self.nbytes
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), self.p, C.c_size_t(self.nbytes), C.c_int(2)) == 0
        return out

    def free(self):
        self.hip.hipFree(self.p)


# ---------------------------------------------------------------- scenes
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
        import sys
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_fuzz
        return test_gpu_fuzz.crowded_scene(pkg, 70, 5)
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


# ---------------------------------------------------------------- RCC:15 + RC:550-576 restated (the test's own arithmetic)
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


def gpu_aov(pkg, api, spec, w, h, frame, tweak=None, seed=1):
    tr = api.create_tracer(0)
    try:
        Setup(pkg, api, tr, spec, w, h, tweak, seed)
        return tr.render_aov(frame)
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. the anchor
def oracle_emitter_frame(pkg, orc, spec, w, h, frame, seed=1):
    ot = orc.create_tracer(8)
    try:
        su = Setup(pkg, orc, ot, spec, w, h, seed=seed)
        su.mgr.RenderFrames(frame)
        return ot.read_frame()[..., :3].copy()  # the frame rendered last: frame `frame`
    finally:
        ot.close()


def palette_index(img, palette):
    """Per pixel: the palette entry whose colour the pixel has exactly, -1 for (0, 0, 0); fails on any other colour."""
    idx = np.full(img.shape[:2], -2, dtype=np.int64)
    idx[(img.view(np.uint32) == 0).all(axis=-1)] = -1
    for k, col in enumerate(palette):
        idx[(img.view(np.uint32) == np.array(col, dtype=F).view(np.uint32)).all(axis=-1)] = k
    assert (idx != -2).all(), f"{int((idx == -2).sum())} pixels are neither a palette colour nor black"
    return idx


@pytest.mark.parametrize("spec", ["emitters", "emitters_dof"])
@pytest.mark.parametrize("frame", [1, 2, 17])
def test_emission_is_the_oracles_frame_of_an_emitter_scene(pkg, api, orc, spec, frame):
    w, h = 64, 36
    palette = emitter_scene(pkg, 0.0)[1]
    want = oracle_emitter_frame(pkg, orc, spec, w, h, frame)
    which = palette_index(want, palette)  # the oracle alone: only palette colours and black, and both occur
    assert (which == -1).any() and len(set(which[which >= 0].tolist())) >= 8, sorted(set(which.ravel().tolist()))
    aov = gpu_aov(pkg, api, spec, w, h, frame)
    assert aov["emission"].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    # object -> palette entry: spheres carry palette[0..2], model i carries palette[3 + i]
    assert np.array_equal(aov["object"], which)
    assert np.array_equal((aov["hit"] & 3) != 0, which >= 0)


# ---------------------------------------------------------------- 5 + 6 + 7. every field, every pixel
FIELD_CASES = [  # name, scene, W, H, frame, tweaks
    ("config2_flat", (2, {}), 64, 36, 1, {}),
    ("config2_flat_f5_nosky", (2, {}), 64, 36, 5, {"useSky": False}),
    ("config3_bvh", (3, {}), 64, 36, 1, {}),
    ("config3_bvh_f9", (3, {}), 48, 27, 9, {}),
    ("glass_balls", "glass_balls_file", 72, 40, 2, {}),
    ("crowded70_many", "crowded70", 64, 36, 3, {}),
    ("config4_dof", (4, {"subdivisions": 3}), 64, 36, 1, {}),
    ("emitters_identity_models", "emitters", 64, 36, 4, {"useSky": True}),
]


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c[0] for c in FIELD_CASES])
def test_every_field_of_every_pixel_equals_the_oracles_functions(pkg, api, orc, case):
    name, spec, w, h, frame, tweak = case
    tr, ot = api.create_tracer(0), orc.create_tracer(1)
    try:
        su = Setup(pkg, api, tr, spec, w, h, tweak)
        so = Setup(pkg, orc, ot, spec, w, h, tweak)
        p = su.params(frame)
        aov = tr.render_aov(frame)
        assert aov.shape == (h, w) and aov.dtype == pkg.abi.AOV_DTYPE
        origins, dirs = camera_rays(orc, p, w, h, frame)
        want = oracle_records(pkg, orc, ot, so, p, origins, dirs, aov["object"])
        want["triangle"] = aov["triangle"]  # (rule 6 below)
        assert_records_equal(aov, want, name)
        hit = aov["hit"] & 3
        assert np.array_equal(aov["object"] >= 0, hit != 0)
        # the restated rays themselves: HIP's own intersection of them is the record
        dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(h, w, 10)
        assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist()
        assert np.array_equal(dbg[..., 0] != 0, hit != 0) and np.array_equal(dbg[..., 1] != 0, (aov["hit"] & 0x100) != 0)
        assert dbg[..., 3:6].view(np.uint32).tolist() == aov["normal"].view(np.uint32).tolist()
        assert dbg[..., 6:9].view(np.uint32).tolist() == aov["pos"].view(np.uint32).tolist()
        # rule 6
        n_tri = check_triangles(orc, so, aov, origins, dirs)
        # rule 7
        cost = tr.render_cost(frame)
        assert np.array_equal(hit, cost[..., 7])
        # the case covers what it is there for
        if spec == (2, {}):
            checker = su.materials["flag"] == pkg.abi.MATERIAL_CHECKERED
            assert checker.any() and checker[aov["object"][hit != 0]].any(), "no checker-flag material in view"
            assert (hit == 0).any() and (aov["object"][hit != 0] < su.n_spheres).any()
        if spec == "glass_balls_file":
            assert (hit == 2).any() and (hit == 1).any()
        if spec == "emitters":
            assert n_tri > 0, "no identity-transform model in view"
        if tweak.get("useSky", su.mgr.useSky) and (hit == 0).any():
            assert aov["albedo"][hit == 0].any()
    finally:
        tr.close()
        ot.close()


# ---------------------------------------------------------------- 8. invariance
def test_device_layout_does_not_change_the_records(pkg, api, monkeypatch):
    out = []
    for layout in ("dense", "pre,arena,cache"):  # the layouts tests/test_gpu_cost_view.py cycles through
        monkeypatch.setenv("RT_LAYOUT", layout)
        out.append(gpu_aov(pkg, api, (3, {}), 96, 54, 3))
        monkeypatch.delenv("RT_LAYOUT")
    assert_records_equal(out[0], out[1], "RT_LAYOUT dense vs pre,arena,cache")
    assert (out[0]["triangle"] >= 0).any()


@pytest.mark.parametrize("spec", [(3, {}), (2, {})], ids=["bvh", "flat"])
@pytest.mark.parametrize("strip_rows", [8, 136])
def test_strip_partitions_reassemble_the_image(pkg, api, spec, strip_rows):
    w, h, frame, parts = 40, 300, 2, 3
    full = gpu_aov(pkg, api, spec, w, h, frame)
    whole = np.zeros_like(full)
    seen = np.zeros(h, dtype=int)
    for i in range(parts):
        tr = api.create_tracer(0)
        try:
            tr.set_partition(strip_rows, i, parts)
            Setup(pkg, api, tr, spec, w, h)
            local = tr.render_aov(frame)
            rows = tr.local_to_global_rows()
            assert local.shape == (len(rows), w)
            whole[rows] = local
            seen[rows] += 1
        finally:
            tr.close()
    assert (seen == 1).all()
    assert_records_equal(whole, full, f"strip_rows {strip_rows}, {parts} parts")
    if strip_rows == 8:
        mt = api.create_multi_tracer([0, 0, 0])
        try:
            Setup(pkg, api, mt, spec, w, h)
            assert_records_equal(mt.render_aov(frame), full, "MultiTracer.render_aov")
        finally:
            mt.close()


@pytest.mark.parametrize("w,h", [(1, 37), (37, 1)])
def test_one_pixel_wide_and_high_images(pkg, api, orc, w, h):
    """uv = 0 / 0 in one direction: every pixel shoots a NaN ray from the camera origin; the record is what rt_debug_intersect gives for it."""
    tr = api.create_tracer(0)
    try:
        su = Setup(pkg, api, tr, (3, {}), w, h)
        aov = tr.render_aov(1)
        origins, dirs = camera_rays(orc, su.params(1), w, h, 1)
        assert np.isnan(dirs).all() and np.isfinite(origins).all()
        dbg = tr.debug_intersect(origins.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(h, w, 10)
        assert dbg[..., 2].view(np.uint32).tolist() == aov["dst"].view(np.uint32).tolist()
        assert np.array_equal(dbg[..., 0] != 0, (aov["hit"] & 3) != 0)
        assert dbg[..., 3:6].view(np.uint32).tolist() == aov["normal"].view(np.uint32).tolist()
        assert dbg[..., 6:9].view(np.uint32).tolist() == aov["pos"].view(np.uint32).tolist()
    finally:
        tr.close()


def test_device_variant_equals_the_host_variant(pkg, api):
    w, h, frame = 96, 54, 3
    for spec in ((3, {}), (2, {}), "crowded70"):
        tr = api.create_tracer(0)
        d = DevBuf(h * w * 64, fill=0xff)
        try:
            su = Setup(pkg, api, tr, spec, w, h)
            host = tr.render_aov(frame)
            su.mgr.RenderFrames(3)  # frames in flight in front of the pass
            tr.render_aov_to_device(frame, d.ptr, d.nbytes)
            tr.synchronize()
            assert_records_equal(d.records(pkg, h, w), host, f"rt_render_aov_to_device vs rt_render_aov ({spec})")
        finally:
            d.free()
            tr.close()


_TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.set_device(0)
root = sys.argv[1]
sys.path.insert(0, root)
import __graft_entry__ as graft
pkg = graft.load_package()
api = pkg.load_library()
w, h, frame = 96, 54, 3
for cfg in (3, 2):
    tr = api.create_tracer(0)
    mgr = pkg.scenes.get(cfg).make_manager(tr, api, w, h)
    mgr.OnEnable(renderSeed=1)
    host = tr.render_aov(frame)
    mgr.RenderFrames(3)
    t = torch.full((h, w, 16), 0x7fc00001, dtype=torch.int32, device="cuda:0")
    tr.render_aov_to_device(frame, t.data_ptr(), t.numel() * 4)
    tr.synchronize()
    dev = t.cpu().numpy().view(pkg.abi.AOV_DTYPE).reshape(h, w)
    assert dev.tobytes() == host.tobytes(), "tensor != host variant (config %d)" % cfg
    # on the caller's stream (rt_set_stream): work enqueued on that stream behind the pass sees its records
    s = torch.cuda.Stream()
    tr.set_stream(s.cuda_stream)
    with torch.cuda.stream(s):
        t2 = torch.zeros((h, w, 16), dtype=torch.int32, device="cuda:0")
        s.synchronize()
        tr.render_aov_to_device(frame, t2.data_ptr(), t2.numel() * 4)
        first = t2[..., 0].clone()
    s.synchronize()
    assert first.cpu().numpy().view(np.uint32).tolist() == host["dst"].view(np.uint32).tolist(), "stream order (config %d)" % cfg
    tr.set_stream(None)
    tr.synchronize()
    tr.close()
print("AOV_TORCH_OK")
"""


def test_device_variant_into_a_torch_tensor(pkg, api):
    """rt_render_aov_to_device(frame, tensor.data_ptr(), ...) == rt_render_aov, and in the order of a torch stream given to
    rt_set_stream.  In a child process that imports torch first, so that the library shares torch's HIP runtime."""
    p = subprocess.run([sys.executable, "-c", _TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "AOV_TORCH_OK" in p.stdout, "rc=%d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


# ---------------------------------------------------------------- 9. no visible state change
def test_aov_calls_leave_no_trace(pkg, api, orc, forced=False):
    cfg, w, h, seed = (3, {}), 96, 54, 5
    snaps, seen = [], {}
    for with_aov in (True, False):
        tr = api.create_tracer(0)
        tr.enable_stats(True)
        su = Setup(pkg, api, tr, cfg, w, h, seed=seed)
        mgr = su.mgr
        t = DevBuf(h * w * 64)

        def probe(tag):
            if with_aov:
                if tag.startswith("after held"):    # (rt_get_counters below launches held frames too: this pass comes first)
                    held_at(tr, "test_gpu_aov: rt_render_aov after held-back frames", forced)
                    met = tr.render_aov(tr.frame())
                before = (tr.frame(), tr.counters())
                a = tr.render_aov(tr.frame())  # the frame the context renders next
                assert_records_equal(a, tr.render_aov(tr.frame()), tag)
                if tag.startswith("after held"):
                    assert_records_equal(a, met, tag)
                tr.render_aov_to_device(1, t.ptr, t.nbytes)
                first = tr.render_aov(1)
                assert_records_equal(first, seen.setdefault(1, first), tag)
                after = (tr.frame(), tr.counters())
                before[1].pop("gpuMs"), after[1].pop("gpuMs")
                assert before == after, tag
        mgr.RenderFrame()                       # frame 1
        probe("after rt_render_frame")
        mgr.RenderFrames(17)                    # frames 2-18: a fused launch, still running when the pass comes
        probe("after rt_render_frames(17)")
        for _ in range(3):                      # frames 19-21: rt_render_frame may hold them back (pending)
            mgr.RenderFrame()
        probe("after held-back frames")
        mgr.RenderFrames(14)                    # frames 22-35, the second of two rt_render_frames calls around a pass
        probe("after the second rt_render_frames")
        c = tr.counters()
        c.pop("gpuMs")
        snaps.append((tr.read_accumulated(), tr.read_frame(), tr.frame(), c))  # (the reads succeed: the watchdog word is clear)
        tr.close()
        t.free()
    (acc_a, frame_a, n_a, c_a), (acc_b, frame_b, n_b, c_b) = snaps
    assert acc_a.tobytes() == acc_b.tobytes() and frame_a.tobytes() == frame_b.tobytes()
    assert n_a == n_b == 36 and c_a == c_b
    ot = orc.create_tracer(16)
    Setup(pkg, orc, ot, cfg, w, h, seed=seed).mgr.RenderFrames(35)
    acc_o = ot.read_accumulated()
    ot.close()
    assert acc_a.view(np.uint32).tobytes() == acc_o.view(np.uint32).tobytes(), "accumulated image != oracle"


def test_aov_calls_leave_no_trace_with_frames_held_back_for_certain(pkg, api, orc, monkeypatch):
    """The same with RT_HOLD_BACK=1: frames 19-21 ARE held back when the AOV pass comes (asserted right before it)."""
    monkeypatch.setenv("RT_HOLD_BACK", "1")
    test_aov_calls_leave_no_trace(pkg, api, orc, forced=True)


# ---------------------------------------------------------------- 10. errors, and the pass's own watchdog word
def test_errors(pkg, api):
    abi = pkg.abi
    buf = np.zeros((36, 64), dtype=abi.AOV_DTYPE)
    dev = DevBuf(buf.nbytes)
    calls = ((api.render_aov, buf.ctypes.data), (api.render_aov_to_device, dev.ptr))
    tr = api.create_tracer(0)
    try:
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_resize
        tr.resize(64, 36)
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_ERR_STATE  # before rt_upload_scene
        Setup(pkg, api, tr, (3, {}), 64, 36)
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes - 64) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, 1, ptr, buf.nbytes + 64) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, 1, None, buf.nbytes) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, 0, ptr, buf.nbytes) == abi.RT_ERR_INVALID_ARG
            assert call(tr.h, -3, ptr, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        # the device variant writes through its pointer: host memory, a misaligned pointer and too small an allocation are refused
        assert api.render_aov_to_device(tr.h, 1, buf.ctypes.data, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_aov_to_device(tr.h, 1, dev.ptr + 4, buf.nbytes) == abi.RT_ERR_INVALID_ARG
        assert api.render_aov_to_device(tr.h, 1, dev.ptr + 64, buf.nbytes) == abi.RT_ERR_INVALID_ARG  # runs past the allocation
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_OK
        tr.synchronize()
        assert (buf["hit"] & 3).any()
        assert_records_equal(dev.records(pkg, 36, 64), buf, "device vs host")
    finally:
        tr.close()
    tr = api.create_tracer(0)
    try:
        tr.resize(64, 36)
        mgr = scene_of(pkg, (3, {})).make_manager(tr, api, 64, 36)
        mgr.InitTexturesAndBuffers()
        mgr.InitBVH()  # a scene, but no rt_set_params yet
        for call, ptr in calls:
            assert call(tr.h, 1, ptr, buf.nbytes) == abi.RT_ERR_STATE
    finally:
        tr.close()
        dev.free()


def test_watchdog_fails_the_pass_not_the_context(pkg, api, monkeypatch):
    """RT_TRAV_LIMIT=4 (read at rt_upload_scene; the step limit is a software counter, nothing can hang): the pass's walks are cut short.
    The host variant says so when it returns, the device variant at the next rt_synchronize, once — and the context's counters and
    images, which no frame of it touched, stay readable.  Every message names the call that reports and, for a deferred report, the
    calls whose pass it was; the next AOV call reports in place of rt_synchronize when it comes first; a pass of another kind
    (rt_query_closest) reports its own word only."""
    tr = api.create_tracer(0)
    t = DevBuf(36 * 64 * 64)
    try:
        monkeypatch.setenv("RT_TRAV_LIMIT", "4")
        su = Setup(pkg, api, tr, (3, {}), 64, 36)
        monkeypatch.delenv("RT_TRAV_LIMIT")
        abi = pkg.abi

        def reported(e, call, *holds):  # the status, the call at the front of the message, and what else it must hold
            msg = str(e.value)
            assert e.value.status == abi.RT_ERR_HIP and "watchdog" in msg, msg
            assert msg.startswith(f"rt status {abi.RT_ERR_HIP}: {call}: "), msg
            for text in holds:
                assert text in msg, (text, msg)
            return msg
        family = "in the AOV pass of an rt_render_aov_to_device, rt_denoise_to_device or rt_reproject_accumulated call"
        for call, name in ((lambda: tr.render_aov(1), "rt_render_aov"), (tr.render_aov_centre, "rt_render_aov_centre")):
            with pytest.raises(abi.RtError) as e:
                call()
            reported(e, name, "a kernel watchdog fired")
        tr.render_aov_to_device(1, t.ptr, t.nbytes)  # enqueued: RT_OK
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()  # reported once
        tr.render_aov_to_device(1, t.ptr, t.nbytes)
        with pytest.raises(abi.RtError) as e:  # the next AOV call reports it if it comes first ...
            tr.render_aov_to_device(1, t.ptr, t.nbytes)
        reported(e, "rt_render_aov_to_device", family)
        tr.synchronize()  # ... once (and the call that reported enqueued nothing)
        tr.render_aov_to_device(1, t.ptr, t.nbytes)
        with pytest.raises(abi.RtError) as e:  # the host variant reports it as well
            tr.render_aov(1)
        reported(e, "rt_render_aov", family)
        tr.synchronize()
        # a pass of another kind neither reports it nor is failed by it: a ray query along the camera's axis says what its own pass met,
        # and the AOV pass is still reported at the next rt_synchronize
        m = np.array(list(su.params(1).camLocalToWorld), dtype=F)
        rays = abi.make_rays(np.tile(m[12:15], (64, 1)), np.tile(m[8:11], (64, 1)))
        tr.render_aov_to_device(1, t.ptr, t.nbytes)
        with pytest.raises(abi.RtError) as e:
            tr.query_closest(rays)
        assert "AOV" not in reported(e, "rt_query_closest", "in this pass", "the records are not valid")
        with pytest.raises(abi.RtError) as e:
            tr.synchronize()
        reported(e, "rt_synchronize", family)
        tr.synchronize()
        c = tr.counters()  # RT_OK: the context's watchdog word was not set
        assert c["segments"] == 0
        assert not tr.read_accumulated().any()
        assert tr.frame() == 1
    finally:
        tr.close()
        t.free()
