"""Non-finite and extreme scene values, case by case: the catalogue tests/test_hazards.py checks on the CPU and tests/test_gpu_hazards.py
renders on the device.  A plain helper module: no GPU, no HIP.

A case is one planted value and the device guard it is aimed at; a base scene is one kernel family.  Every (case, base) that applies is
rendered the same way by every tracer (the HIP library's, the oracle's, the reference text's): Rig builds the arrays and the RtParams a
tracer is given, drive() uploads them and renders two single frames and one fused launch of three.  The manager mirror is used to BUILD
the records (its transforms, the BVH builder) and is then left aside: its UpdateModels would write the planted matrices over, and its
numpy inverse refuses some of them.

What a value does to the three per-launch tables of the FLAT kernel (the `tables` of a case, asserted on the flat-tables base only; every
other base is outside the caps and reports (0, 0, 0)) is reasoned here from the rule of rt_primary.h, "switched on only when every entry
is finite", applied to the fp32 quantities the table holds, never read off the device:

  off  the planted value makes an entry of the table of origin constants non-finite in fp32: a sphere record (centre, r * r, |c|^2 - r * r),
       the camera origin or its square, a model-space origin worldToLocal * o, or it turns the no-defocus raygen off.  The two per-tile
       tables ride on that table, so all three debug calls report 0.
  on   every entry stays finite.  The per-tile tables are then read; where one of their own inputs is not finite (tile_cand_finite) they
       keep every bit, which no debug call shows: the image, the exact counters and filter_violations == 0 are the check there.

  A radius of 1e20 is finite, its square is not (fp32: 1e40 = inf) and the sphere records hold r * r: `off`.  radius 1e15 is the case of
  a huge sphere whose records stay finite: `on`, and its bit must survive in every tile (it contains the camera)."""
import os
import sys

import numpy as np

import capfuzz_scenes as cs

NAN, INF = float("nan"), float("inf")
BASES = ("flat-tables", "flat-general", "bvh", "many")
# (W, H): none above 48 x 32, none a multiple of the 8 x 8 tile in both directions but flat-general's (pooled at RT_POOL_MIN_ITEMS=0)
SIZES = {"flat-tables": (43, 27), "flat-general": (48, 32), "bvh": (41, 23), "many": (45, 30)}
# capfuzz seeds whose objects the camera sees: seed 22 (4 models of 4 triangles) with 5 spheres, within every cap; seed 13 with 33 spheres and
# 17 triangles in 3 models, over two caps
FLAT_TABLES_SEED, FLAT_GENERAL_SEED = 22, 13
GUARDS = ("invert_affine", "primary_fill", "tile_cand_finite", "sphere_pretest", "model_box_step", "minmax_nan", "math_classes",
          "shared_reciprocal")
# other device code a value is aimed at, beyond the eight guards above
OTHER_GUARDS = ("shade", "raygen", "sky", "accumulate")
FRAME_TOP = 2**31 - 1 - 5   # five frames from here leave the context's frame counter at INT32_MAX, the last value an int holds


class Targets:
    """which sphere, which model and which material of a base scene a value is planted in: objects the camera sees"""

    def __init__(self, sphere, model, material_on):
        self.sphere, self.model, self.material_on = sphere, model, material_on

    def material(self, sc):
        return sc.spheres[self.sphere].material if self.material_on == "sphere" else sc.models[self.model].material


TARGETS = {"flat-tables": Targets(3, 3, "sphere"), "flat-general": Targets(12, 0, "sphere"), "bvh": Targets(None, 7, "model"),
           "many": Targets(1, 1, "model")}


def base_scene(pkg, base):
    """-> (SceneDescription, render seed, (W, H)), a fresh one per call (a case writes into it)"""
    if base == "flat-tables":
        sc, seed = cs._build(pkg, FLAT_TABLES_SEED, n_spheres=5)
    elif base == "flat-general":
        sc, seed = cs._build(pkg, FLAT_GENERAL_SEED, n_spheres=33, split=(12, 2, 3))
    elif base == "bvh":   # config 3's kind (inner roots: the root filter and the hot cache), fewer rays per pixel, and without the
        sc, seed = pkg.scenes.get(3), 5   # room's back wall: a sky hazard needs a ray that leaves the scene
        sc.settings.update(numRaysPerPixel=2, maxBounceCount=5)
        sc.models = [m for m in sc.models if m.name != "WallBack"]
    elif base == "many":   # more than 64 models: the two-level filter
        here = os.path.dirname(os.path.abspath(__file__))
        if here not in sys.path:
            sys.path.insert(0, here)
        import test_gpu_fuzz
        sc, seed = test_gpu_fuzz.crowded_scene(pkg, 70, 5), 11
    else:
        raise KeyError(base)
    # every base has the sky on and the sun above the horizon (the default direction is straight down: never seen), so that a sky
    # hazard changes what the camera sees
    sc.settings.update(useSky=True, sunFocus=500.0, sunIntensity=10.0, sunTransform=pkg.manager.Transform((0, 0, 0), (50, -30, 0)))
    return sc, seed, SIZES[base]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

class Case:
    """name; kind (what it needs of a base: "sphere" needs spheres); guard; tables ("on" / "off": see the module text); the plant, at
    one of three levels: scene(pkg, sc, t) on the objects, records(pkg, models, spheres, t) on the RtModel / RtSphere records after
    the mirror filled them, params(rig) on the RtParams (and rig.frame0)"""

    def __init__(self, name, kind, guard, tables="on", scene=None, records=None, params=None, saturating=False, note=""):
        assert guard in GUARDS + OTHER_GUARDS and tables in ("on", "off")
        self.name, self.kind, self.guard, self.tables = name, kind, guard, tables
        self.scene, self.records, self.params = scene, records, params
        self.saturating, self.note = saturating, note
        self.refused = None   # no record of the catalogue is refused by rt_upload_scene: it validates offsets and trees, not values

    def applies(self, base):
        return TARGETS[base].sphere is not None if self.kind == "sphere" else True


def _sphere(**kw):
    def plant(pkg, sc, t):
        s = sc.spheres[t.sphere]
        c = list(s.centre)
        for k, v in kw.items():
            if k == "radius":
                s.radius = float(v)
            else:
                c["xyz".index(k)] = float(v)
        s.centre = tuple(c)
    return plant


def _material(**kw):
    def plant(pkg, sc, t):
        m = t.material(sc)
        for k, v in kw.items():
            assert hasattr(m, k), k
            setattr(m, k, v)
    return plant


def _glass(**kw):
    return _material(flag=2, smoothness=1.0, specularProbability=1.0, **kw)


def _emitter(strength):
    return _material(emissionCol=(1.0, 0.9, 0.7, 1.0), emissionStrength=strength)


def _setting(beside=False, **kw):
    """beside: the value leaves the camera rays in the camera's own plane (a focus plane of no extent or at no distance: the direction is
    the jitter alone), where the base scenes have nothing; the target sphere is moved into that plane, 1.5 radii beside the camera, so
    that such rays meet an object a per-tile table could wrongly have dropped"""
    def plant(pkg, sc, t):
        if beside and t.sphere is not None:
            tf = sc.camera.transform
            right = tf.rotation_matrix()[:, 0]
            sc.spheres[t.sphere].centre = tuple(float(p + 1.5 * r) for p, r in zip(tf.position, right))
            sc.spheres[t.sphere].radius = 1.0
        for k, v in kw.items():
            assert k in sc.settings or k in ("defocusStrength", "focusDistance", "sunFocus", "sunIntensity", "useSky"), k
            sc.settings[k] = v
    return plant


def _transform(position=None, mirror=False):
    def plant(pkg, sc, t):
        tf = sc.models[t.model].transform
        if position is not None:
            tf.position = tuple(float(v) for v in position(tf.position))
        if mirror:   # reflected through the plane x = the camera's x: the determinant changes sign and (a cube is its own mirror image) the model moves
            m = np.eye(4)
            m[0, 0], m[0, 3] = -1.0, 2.0 * sc.camera.transform.position[0]
            sc.models[t.model].transform = pkg.manager.MatrixTransform(m @ tf.localToWorldMatrix)
    return plant


def _to_abi(m):
    """4 x 4 (row, col) float64 -> the 16 floats of an RtModel matrix (manager.matrix_to_abi)"""
    return (np.asarray(m, dtype=np.float64).T.reshape(16) + 0.0).astype(np.float32)


def _from_abi(a):
    return np.asarray(a, dtype=np.float64).reshape(4, 4).T.copy()


def matrix_pair(l2w, what):
    """the (localToWorld, worldToLocal) records of a matrix hazard, from a regular localToWorld: both computed in float64 and rounded once"""
    l2w = np.array(l2w, dtype=np.float64)
    if what == "singular":   # one zero column; worldToLocal is the pseudo-inverse (one zero row): what a host would compute for a flattened model
        l2w[:3, 0] = 0.0
        w2l = np.eye(4)
        w2l[:3, :3] = np.linalg.pinv(l2w[:3, :3])
        w2l[:3, 3] = -w2l[:3, :3] @ l2w[:3, 3]
    elif what == "nan":
        w2l = np.linalg.inv(l2w)
        w2l[0, 0] = NAN
        l2w[0, 0] = NAN
    else:
        l2w[:3, :3] *= float(what)
        w2l = np.linalg.inv(l2w)
    return _to_abi(l2w), _to_abi(w2l)


def _matrix(what):
    def plant(pkg, models, spheres, t):
        l2w, w2l = matrix_pair(_from_abi(models[t.model]["localToWorld"]), what)
        models[t.model]["localToWorld"], models[t.model]["worldToLocal"] = l2w, w2l
    return plant


def _camera(**kw):
    def plant(rig):
        for k, v in kw.items():
            rig.p.camLocalToWorld[12 + "xyz".index(k)] = v
    return plant


def _plane_overflow(rig):
    # ViewParams written directly: what a field of view a hair short of 180 degrees gives at a focus distance of 1e35: the plane's extents
    # 2 f tan(fov / 2) leave fp32, its distance stays finite
    rig.p.viewParams[0], rig.p.viewParams[1], rig.p.viewParams[2] = INF, INF, 1e35


def _spp_minimum(rig):
    rig.p.numRaysPerPixel = 0   # rt_render_frame refuses < 0


def _frame_top(rig):
    rig.frame0 = FRAME_TOP


CASES = [
    # spheres: the packed two-sphere pre-test (camera rays with the table, every ray without) and the general loop's shared reciprocal
    Case("radius-1e20", "sphere", "shared_reciprocal", "off", scene=_sphere(radius=1e20), note="r * r = inf in the sphere records"),
    Case("radius-1e15", "sphere", "tile_cand_finite", "on", scene=_sphere(radius=1e15), note="r * r = 1e30: every record finite; the bit stays in every tile"),
    Case("radius-1e19-ground", "sphere", "sphere_pretest", "on", scene=_sphere(y=-1e19, radius=1e19),
         note="a ground sphere whose top is at y = 0: |c|^2, r * r and (2 off.d)^2 sit at the edge of fp32 (1e38), their differences cancel"),
    Case("radius-0", "sphere", "sphere_pretest", "on", scene=_sphere(radius=0.0)),
    Case("radius-negative", "sphere", "sphere_pretest", "on", scene=_sphere(radius=-1.0)),
    Case("radius-nan", "sphere", "sphere_pretest", "off", scene=_sphere(radius=NAN)),
    Case("radius-inf", "sphere", "sphere_pretest", "off", scene=_sphere(radius=INF)),
    Case("radius-1e-30", "sphere", "shared_reciprocal", "on", scene=_sphere(radius=1e-30), note="r * r underflows to 0"),
    Case("centre-nan", "sphere", "primary_fill", "off", scene=_sphere(x=NAN)),
    Case("centre-1e30", "sphere", "sphere_pretest", "off", scene=_sphere(y=1e30), note="|c|^2 = inf"),
    Case("centre-inf", "sphere", "primary_fill", "off", scene=_sphere(z=INF)),
    # models: the packed two-model box step, the root filter
    Case("model-mirrored", "model", "model_box_step", "on", scene=_transform(mirror=True)),
    Case("model-position-1e20", "model", "model_box_step", "on", scene=_transform(position=lambda p: (p[0], 1e20, p[2])),
         note="worldToLocal * o is about 1e20: finite"),
    Case("model-position-nan", "model", "minmax_nan", "off", scene=_transform(position=lambda p: (NAN, p[1], p[2]))),
    Case("matrix-singular", "matrix", "invert_affine", "on", records=_matrix("singular"),
         note="the root filter of this model is dropped; nothing exposes that per model: the image and filter_violations are the check"),
    Case("matrix-scale-1e-20", "matrix", "invert_affine", "on", records=_matrix(1e-20), note="worldToLocal about 1e20: the model-space origin stays finite"),
    Case("matrix-scale-1e15", "matrix", "model_box_step", "on", records=_matrix(1e15)),
    Case("matrix-nan-entry", "matrix", "minmax_nan", "off", records=_matrix("nan")),
    # materials: the shade block
    Case("smoothness-2", "material", "shade", scene=_material(smoothness=2.0, specularProbability=1.0)),
    Case("smoothness-negative", "material", "shade", scene=_material(smoothness=-1.0, specularProbability=1.0)),
    Case("smoothness-nan", "material", "shade", scene=_material(smoothness=NAN, specularProbability=1.0)),
    Case("specular-probability-nan", "material", "shade", scene=_material(specularProbability=NAN, smoothness=0.7)),
    Case("specular-probability-2", "material", "shade", scene=_material(specularProbability=2.0, smoothness=0.7)),
    Case("glass-ior-0", "glass", "shade", scene=_glass(ior=0.0)),
    Case("glass-ior-inf", "glass", "shade", scene=_glass(ior=INF)),
    Case("glass-ior-nan", "glass", "shade", scene=_glass(ior=NAN)),
    Case("glass-ior-1", "glass", "shade", scene=_glass(ior=1.0)),
    Case("emission-inf", "material", "shade", scene=_emitter(INF)),
    Case("emission-1e38", "material", "shade", scene=_emitter(1e38)),
    Case("diffuse-0", "material", "shade", scene=_material(diffuseCol=(0.0, 0.0, 0.0, 1.0), specularProbability=0.0)),
    Case("diffuse-out-of-range", "material", "shade", scene=_material(diffuseCol=(-0.5, 1.5, 2.0, 1.0), specularProbability=0.0)),
    Case("diffuse-nan", "material", "shade", scene=_material(diffuseCol=(NAN, 0.5, 0.5, 1.0), specularProbability=0.0)),
    Case("glass-absorption-inf", "glass", "math_classes", scene=_glass(ior=1.5, absorption=(INF, 0.5, 0.0, 1.0), absorptionMultiplier=1.0),
         note="exp(-inf), and exp(-(0 * inf))"),
    Case("glass-absorption-multiplier-negative", "glass", "math_classes", scene=_glass(ior=1.5, absorption=(1.0, 0.5, 0.25, 1.0), absorptionMultiplier=-50.0),
         note="exp of a large positive argument"),
    Case("checkered", "material", "shade", scene=_material(flag=1, diffuseCol=(0.1, 0.4, 0.9, 1.0), emissionCol=(0.9, 0.2, 0.1, 1.0), specularProbability=0.0),
         note="both colours of the pattern are new: whichever square a hit lies in, it changes"),
    # settings
    Case("diverge-inf", "setting", "tile_cand_finite", "on", scene=_setting(beside=True, divergeStrength=INF), note="the jitter bound is not finite: every tile keeps every bit"),
    Case("diverge-1e30", "setting", "tile_cand_finite", "on", scene=_setting(beside=True, divergeStrength=1e30),
         note="the tile's cone has no finite sine: every sphere stays; the rays lie in the camera's plane and meet the sphere moved there"),
    Case("diverge-5e20", "setting", "tile_cand_finite", "on", scene=_setting(beside=True, divergeStrength=5e20),
         note="the jitter is about 1.1e19 per pixel: the rays stay finite (|d|^2 < 3.4e38) while the square of the tile's bound, twice as long, "
              "is inf; the sine tests are not finite and the sphere moved into the camera's plane must stay"),
    Case("focus-distance-0", "setting", "tile_cand_finite", "on", scene=_setting(beside=True, focusDistance=0.0),
         note="a plane of no extent at no distance (L2 = 0): every tile keeps every bit; the rays lie in the camera's plane and meet the sphere moved there"),
    Case("defocus-inf", "setting", "raygen", "off", scene=_setting(defocusStrength=INF), note="defocus != 0: the literal raygen, no table"),
    Case("sun-focus-0", "setting", "math_classes", scene=_setting(sunFocus=0.0), note="the exponent 1000 / sunFocus is inf: pow(x, inf)"),
    Case("sun-focus-1e30", "setting", "math_classes", scene=_setting(sunFocus=1e30), note="pow(x, 1e-27)"),
    Case("sun-intensity-inf", "setting", "sky", scene=_setting(sunIntensity=INF), saturating=True),
    Case("bounces-0", "setting", "shade", scene=_setting(maxBounceCount=0)),
    # camera and parameters, through RtParams
    Case("camera-position-1e20", "param", "primary_fill", "off", params=_camera(x=1e20), note="|o|^2 = inf"),
    Case("camera-position-nan", "param", "primary_fill", "off", params=_camera(y=NAN), note="a camera matrix that is not finite: the literal raygen"),
    Case("plane-extents-overflow", "param", "tile_cand_finite", "on", params=_plane_overflow),
    Case("rays-per-pixel-minimum", "param", "accumulate", "on", params=_spp_minimum, saturating=True, note="0 rays: 0 / 0 in every pixel"),
    Case("frame-index-top", "param", "raygen", "on", params=_frame_top),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the side passes: every kind of object hazard (a sphere's radius and centre, a model's matrix records, every material field), >= 12
SIDE_CASES = ("radius-1e20", "radius-0", "radius-nan", "centre-nan", "centre-1e30", "model-position-nan", "matrix-singular", "matrix-scale-1e-20",
              "matrix-nan-entry", "smoothness-nan", "glass-ior-0", "glass-ior-nan", "emission-inf", "diffuse-nan", "glass-absorption-inf")
SIDE_BASES = ("flat-general", "bvh", "many")
# rt_nee_trace: the four emission and area hazards (a zero-radius emissive sphere and a singular emissive model are built by the test)
NEE_CASES = ("emission-inf", "emission-1e38", "radius-0", "matrix-singular")


def table(cases=CASES):
    """the catalogue as text: case x guard x tables x base scene"""
    rows = [f"{'case':38s} {'guard':18s} {'tables':6s} " + " ".join(f"{b:12s}" for b in BASES) + " marks"]
    for c in cases:
        marks = ", ".join(m for m, on in (("saturating", c.saturating), ("refused", c.refused is not None)) if on)
        rows.append(f"{c.name:38s} {c.guard:18s} {c.tables:6s} " + " ".join(f"{'x' if c.applies(b) else '-':12s}" for b in BASES) + " " + marks)
    return "\n".join(rows)


# ---- building and driving -------------------------------------------------------------------------------------------------------------

class _NoTracer:
    def __getattr__(self, name):
        raise AssertionError(f"the tracer is not to be called ({name})")


class Rig:
    """what a tracer is given for (base, case): the arrays of rt_upload_scene and the RtParams.  `builder` is a library with the BVH
    builder and rt_camera_view_params (the HIP library or the oracle: the same bytes); case None = the unplanted base scene."""

    def __init__(self, pkg, builder, base, case=None):
        sc, seed, (w, h) = base_scene(pkg, base)
        t = TARGETS[base]
        assert case is None or case.applies(base)
        if case is not None and case.scene:
            case.scene(pkg, sc, t)
        mgr = sc.make_manager(_NoTracer(), builder, w, h)
        mgr.renderSeed = seed
        with np.errstate(all="ignore"):
            data = mgr.CreateAllMeshData(mgr.models)
        self.models, self.triangles, self.nodes = data["meshInfo"].copy(), data["triangles"], data["nodes"]
        self.spheres = mgr._pack_spheres()
        if case is not None and case.records:
            case.records(pkg, self.models, self.spheres, t)
        self.p = mgr.params()
        self.frame0 = 1
        if case is not None and case.params:
            case.params(self)
        self.base, self.case, self.w, self.h, self.targets = base, case, w, h, t
        self.tri_count = np.array([m.Mesh.triangle_count for m in mgr.models], dtype=np.int64)
        self.materials = np.concatenate([self.spheres["material"], self.models["material"]])   # by object index: spheres first
        self.n_spheres = len(self.spheres)

    def params(self, frame_offset=0):
        self.p.frame = self.frame0 + frame_offset
        return self.p

    def upload(self, tr):
        tr.resize(self.w, self.h)
        tr.upload_scene(self.models, self.triangles, self.nodes, self.spheres)
        tr.set_params(self.params())
        tr.reset_accumulation()


def drive(rig, tr, fused=3):
    """tests/test_gpu_geometry.py's drive without the manager: two single frames, then one rt_render_frames(fused).
    -> ((acc, frame) after the single frames, (acc, frame) at the end, the counters)"""
    rig.upload(tr)
    for i in range(2):
        tr.set_params(rig.params(i))
        tr.render_frame()
    single = (tr.read_accumulated().copy(), tr.read_frame().copy())
    tr.set_params(rig.params(2))
    tr.render_frames(fused)
    return single, (tr.read_accumulated().copy(), tr.read_frame().copy()), tr.counters()


def assert_image(got, want, what):
    """tests/test_gpu_geometry.py's rule: bit for bit; where the expected image holds NaN, the NaN positions are compared and every
    other value bit for bit (a NaN's sign and payload are not part of the contract)"""
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ ({int(np.isnan(got).sum())} values against {int(nan.sum())} expected)"
    same = got[~nan].view(np.uint32) == want[~nan].view(np.uint32)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} non-NaN values differ"


def same_image(a, b):
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def nan_share(img):
    """share of the pixels with a NaN colour"""
    return float(np.isnan(img[..., :3]).any(axis=-1).mean())


_expected = {}


def expected(pkg, orc, base, case):
    """the oracle's drive() of (base, case): computed once, shared, never written"""
    key = (base, case.name if case else None)
    if key not in _expected:
        tr = orc.create_tracer(8)
        try:
            out = drive(Rig(pkg, orc, base, case), tr)
        finally:
            tr.close()
        for part in out[:2]:
            for img in part:
                img.setflags(write=False)
        _expected[key] = out
    return _expected[key]


def pixel_centre_rays(rig):
    """one ray per pixel centre, (H, W, 3) origins and directions in fp32: through the view plane as RC:557-558 places it, without jitter"""
    F = np.float32
    m = np.array(list(rig.p.camLocalToWorld), dtype=F)
    vp = np.array(list(rig.p.viewParams), dtype=F)
    with np.errstate(all="ignore"):
        u = (np.arange(rig.w, dtype=F) / F(rig.w - 1) - F(0.5)) * vp[0]
        v = (np.arange(rig.h, dtype=F) / F(rig.h - 1) - F(0.5)) * vp[1]
        U, V = np.meshgrid(u, v)
        Z = np.full(U.shape, vp[2], dtype=F)
        focus = [m[r] * U + m[4 + r] * V + m[8 + r] * Z + m[12 + r] for r in range(3)]
        origin = np.broadcast_to(m[12:15], U.shape + (3,)).astype(F)
        d = np.stack(focus, axis=-1).astype(F) - origin
        d = (d / np.sqrt((d * d).sum(axis=-1, keepdims=True), dtype=F)).astype(F)
    return np.ascontiguousarray(origin), np.ascontiguousarray(d)
