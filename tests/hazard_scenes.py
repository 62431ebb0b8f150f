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
  a huge sphere whose records stay finite: `on`, and its bit must survive in every tile (it contains the camera).

  A triangle's entry is vro = worldToLocal * o - A and d = dot(vro, AB x AC).  The "one" cases plant in C (and B), never in A, so vro stays
  finite and d decides.  C += 1e15 leaves one long edge: the face is about 1e15 |AB| and d about 1e16, finite: `on`.  So it is for the
  mesh's vertex at 1e15 and at 3e19 (where that mesh builds): the flat-tables meshes are soups, the vertex is corner C of one triangle
  and of no other, and 3e19 |AB| |vro| is about 1e21.  One long edge cannot take the face out of fp32
  (3.4e38 / 1e20 is far above any |AB| of a base scene), so tri-vertex-1e20 makes two: C = C * 1e20 + 1e20 and B.x += 1e20 give the face
  components 1e20 * 1e20 = inf without an inf - inf: d is not finite, `off`.  A NaN or inf coordinate of C reaches d through the face:
  `off`.  A degenerate, collinear, tiny or flat triangle has a face of 0 or a denormal and d = 0: finite, `on`; so are all normals, which
  no table holds.  tests/test_hazards.py restates the rule in fp32 on the flat-tables records of every triangle and mesh case and
  compares it with this column."""
import ctypes as C
import copy
import os
import sys

import numpy as np

import capfuzz_scenes as cs
from fuzz_scenes import crowded_overflow_scene

NAN, INF = float("nan"), float("inf")
BASES = ("flat-tables", "flat-general", "bvh", "many")
# (W, H): none above 48 x 32, none a multiple of the 8 x 8 tile in both directions but flat-general's (pooled at RT_POOL_MIN_ITEMS=0).
# flat-tables: its camera barely sees its four models; at 45 x 29 the most seen triangle is the first hit of 5 pixel-centre rays (at
# 43 x 27 of 3, under SEEN_FLOOR)
SIZES = {"flat-tables": (45, 29), "flat-general": (48, 32), "bvh": (41, 23), "many": (45, 30)}
# capfuzz seeds whose objects the camera sees: seed 22 (4 models of 4 triangles) with 5 spheres, within every cap; seed 13 with 33 spheres and
# 17 triangles in 3 models, over two caps
FLAT_TABLES_SEED, FLAT_GENERAL_SEED = 22, 13
GUARDS = ("invert_affine", "primary_fill", "tile_cand_finite", "sphere_pretest", "model_box_step", "minmax_nan", "math_classes",
          "shared_reciprocal",
          # the triangles themselves: tri_test's threshold and strict <, primary_fill's triangle entries, tile_tri_mask's keep rule, the
          # leaf-root box, box_dst on bounds a vertex made NaN / huge / flat, resolve_hit's two normalisations, the two BVH builders
          "tri_eps", "tri_primary", "tile_tri_finite", "leaf_root_box", "box_dst", "resolve_normal", "bvh_build")
# other device code a value is aimed at, beyond the guards above (light_area: the light table's area rule, through NEE_TRI_CASES)
OTHER_GUARDS = ("shade", "raygen", "sky", "accumulate", "light_area")
FRAME_TOP = 2**31 - 1 - 5   # five frames from here leave the context's frame counter at INT32_MAX, the last value an int holds


class Targets:
    """which sphere, which model and which material of a base scene a value is planted in: objects the camera sees.  The triangle
    hazards have a model of their own (tri_model: `model` where one of its triangles is the first hit of SEEN_FLOOR pixel-centre rays,
    otherwise the model of the scene's most seen triangle) and in it the seen triangle: aim() works both out from the oracle's first hits of the
    unplanted scene.  Models that share a mesh share their triangle records: a value planted in them is seen through every one."""

    def __init__(self, sphere, model, material_on, tri_model=None):
        self.sphere, self.model, self.material_on, self.tri_model = sphere, model, material_on, tri_model
        self.seen = None   # aim(): the index of the seen triangle in the uploaded array of the unplanted scene
        self.seen_count = self.seen_corners = self.most_seen = None

    def material(self, sc):
        return sc.spheres[self.sphere].material if self.material_on == "sphere" else sc.models[self.model].material


TARGETS = {"flat-tables": Targets(3, 3, "sphere"), "flat-general": Targets(12, 0, "sphere"), "bvh": Targets(None, 7, "model"),
           "many": Targets(1, 1, "model")}
SEEN_FLOOR = 4   # pixel-centre rays whose first hit the seen triangle is, at least: tests/test_many_models.py's floor for its witnesses


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
        sc, seed = crowded_overflow_scene(pkg, 70, 5), 11
    else:
        raise KeyError(base)
    # every base has the sky on and the sun above the horizon (the default direction is straight down: never seen), so that a sky
    # hazard changes what the camera sees
    sc.settings.update(useSky=True, sunFocus=500.0, sunIntensity=10.0, sunTransform=pkg.manager.Transform((0, 0, 0), (50, -30, 0)))
    return sc, seed, SIZES[base]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

class Case:
    """name; kind (what it needs of a base: "sphere" needs spheres); guard; tables ("on" / "off": see the module text); the plant, at
    one of four levels: scene(pkg, sc, t) on the objects, triangles(pkg, rig, t) on a copy of the RtTriangle records right after the
    mirror built them (values only: the trees and their bounds stay those of the unplanted mesh), records(pkg, models, spheres, t) on
    the RtModel / RtSphere records after the mirror filled them, params(rig) on the RtParams (and rig.frame0).
    refused: {base: who refuses it}; no record of the catalogue is refused by rt_upload_scene (it validates offsets and trees, not
    values), but the BVH builders refuse a mesh whose split costs overflow, and Rig then has .refused set and no arrays"""

    def __init__(self, name, kind, guard, tables="on", scene=None, triangles=None, records=None, params=None, saturating=False, note="",
                 refused=None):
        assert guard in GUARDS + OTHER_GUARDS and tables in ("on", "off")
        self.name, self.kind, self.guard, self.tables = name, kind, guard, tables
        self.scene, self.triangles, self.records, self.params = scene, triangles, records, params
        self.saturating, self.note = saturating, note
        self.refused = dict(refused) if refused else None

    def applies(self, base):
        return TARGETS[base].sphere is not None if self.kind == "sphere" else True

    def builds(self, base):
        return self.applies(base) and not (self.refused and base in self.refused)


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


F32 = np.float32
POS, NORM = ("posA", "posB", "posC"), ("normA", "normB", "normC")


def _tri_all(write):
    """write(T) on the records of every triangle of the target model (a view: written in place), all arithmetic in fp32"""
    def plant(pkg, rig, t):
        lo = int(rig.models["triOffset"][t.tri_model])
        with np.errstate(all="ignore"):
            write(rig.triangles[lo:lo + int(rig.tri_count[t.tri_model])])
    return plant


def _tri_one(write):
    """write(T) on the one record of the seen triangle"""
    def plant(pkg, rig, t):
        assert np.array_equal(np.stack([rig.triangles[p][t.seen] for p in POS]), t.seen_corners), "the seen triangle is where aim() found it"
        with np.errstate(all="ignore"):
            write(rig.triangles[t.seen:t.seen + 1])
    return plant


def _w_degenerate(T):
    T["posC"] = T["posA"]


def _w_collinear(T):
    T["posC"] = T["posA"] + (T["posB"] - T["posA"]) / F32(2)


def _w_sliver(T):
    T["posC"] = T["posA"] + (T["posB"] - T["posA"]) / F32(2) + F32(1e-4) * (T["posC"] - T["posA"])


def _w_tiny(k):
    def write(T):
        T["posB"] = T["posA"] + F32(k) * (T["posB"] - T["posA"])
        T["posC"] = T["posA"] + F32(k) * (T["posC"] - T["posA"])
    return write


def _w_flipped(T):
    for b, c in (("posB", "posC"), ("normB", "normC")):
        T[b], T[c] = T[c].copy(), T[b].copy()


def _w_coincident(T):
    for i in range(1, len(T), 2):
        for p, n in zip(POS, NORM):
            T[p][i], T[n][i] = T[p][i - 1], -T[n][i - 1]


def _w_c_1e15(T):
    T["posC"] = T["posC"] + F32(1e15)


def _w_two_edges_1e20(T):
    T["posC"] = T["posC"] * F32(1e20) + F32(1e20)
    T["posB"][:, 0] = T["posB"][:, 0] + F32(1e20)


def _w_component(field, axis, value):
    def write(T):
        T[field][:, axis] = value
    return write


def _w_normals(k):
    def write(T):
        for n in NORM:
            T[n] = T[n] * F32(k)
    return write


def _w_normals_opposed(T):
    T["normB"] = -T["normA"]
    T["normC"] = -T["normA"]


def seen_vertex(mesh, corners, which=2):
    """the index in `mesh` of corner `which` (0, 1, 2 = A, B, C) of the triangle whose uploaded corners are `corners`: the builders keep a
    triangle's corner order"""
    tri = mesh.triangles.reshape(-1, 3)
    hit = [k for k in range(len(tri)) if np.array_equal(mesh.vertices[tri[k]], corners)]
    assert hit, "the seen triangle is a triangle of the target model's mesh"
    return int(tri[hit[0]][which])


def _mesh(write):
    """write(mesh, v) on a deep copy of the target model's mesh, v = the index of corner C of the seen triangle: the builders, the leaf-root
    box, the root filter and every node's bounds see the value"""
    def plant(pkg, sc, t):
        m = sc.models[t.tri_model]
        m.Mesh = copy.deepcopy(m.Mesh)
        with np.errstate(all="ignore"):
            write(m.Mesh, seen_vertex(m.Mesh, t.seen_corners))
    return plant


def _m_add(k):
    def write(mesh, v):
        mesh.vertices[v] = mesh.vertices[v] + F32(k)
    return write


def _m_set(k):
    def write(mesh, v):
        mesh.vertices[v] = F32(k)
    return write


def _m_component(axis, value):
    def write(mesh, v):
        mesh.vertices[v, axis] = value
    return write


def _m_flat(mesh, v):
    mesh.vertices[:, 1] = mesh.vertices[0, 1]


def _m_point(mesh, v):
    mesh.vertices[:] = mesh.vertices[0]


def _m_scale(k):
    def write(mesh, v):
        mesh.vertices[:] = mesh.vertices * F32(k)
    return write


_BUILDERS_REFUSE = {"bvh": "build_bvh", "many": "build_bvh"}   # RT_ERR_SCENE: split costs that overflow; the FLAT bases' meshes build


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
    # the triangle records, every triangle of the target model: tri_test's determinant threshold and strict <, tile_tri_mask's keep rule
    Case("tri-degenerate", "triangle", "tri_eps", "on", triangles=_tri_all(_w_degenerate), note="C = A: AB x AC = 0, the determinant is 0"),
    Case("tri-collinear", "triangle", "tile_tri_finite", "on", triangles=_tri_all(_w_collinear), note="C = A + (B - A) / 2"),
    Case("tri-sliver", "triangle", "tri_eps", "on", triangles=_tri_all(_w_sliver), note="C = A + (B - A) / 2 + 1e-4 (C - A)"),
    Case("tri-tiny-1e-4", "triangle", "tri_eps", "on", triangles=_tri_all(_w_tiny(1e-4)),
         note="B and C pulled to A by 1e-4: |determinant| straddles 1E-8 across the image"),
    Case("tri-tiny-1e-20", "triangle", "tri_eps", "on", triangles=_tri_all(_w_tiny(1e-20)), note="the same by 1e-20: AB x AC underflows to 0"),
    Case("tri-flipped", "triangle", "tri_eps", "on", triangles=_tri_all(_w_flipped), note="B <-> C: the winding; with culling on the model vanishes"),
    Case("tri-coincident", "triangle", "tri_eps", "on", triangles=_tri_all(_w_coincident),
         note="every odd triangle = its predecessor's corners with negated normals: equal dst, the strict < keeps the first in walk order"),
    # the seen triangle alone
    Case("tri-vertex-1e15", "triangle", "tile_tri_finite", "on", triangles=_tri_one(_w_c_1e15), note="C += 1e15: one long edge, the face about 1e15 |AB|, d finite"),
    Case("tri-vertex-1e20", "triangle", "tri_primary", "off", triangles=_tri_one(_w_two_edges_1e20),
         note="C = C * 1e20 + 1e20 and B.x += 1e20: two long edges, face components 1e40 = inf (C alone leaves the face at 1e20 |AB|: finite)"),
    Case("tri-vertex-nan", "triangle", "tri_primary", "off", triangles=_tri_one(_w_component("posC", 0, NAN))),
    Case("tri-vertex-inf", "triangle", "tri_primary", "off", triangles=_tri_one(_w_component("posC", 1, INF))),
    # the vertex normals: resolve_hit normalises the interpolated normal twice
    Case("tri-normals-zero", "triangle", "resolve_normal", "on", triangles=_tri_all(_w_normals(0.0)), note="normalize(0)"),
    Case("tri-normal-nan", "triangle", "resolve_normal", "on", triangles=_tri_all(_w_component("normA", 1, NAN))),
    Case("tri-normals-1e20", "triangle", "resolve_normal", "on", triangles=_tri_all(_w_normals(1e20)), note="the squared length is inf"),
    Case("tri-normals-1e-30", "triangle", "resolve_normal", "on", triangles=_tri_all(_w_normals(1e-30)), note="the squared length is 0"),
    Case("tri-normals-opposed", "triangle", "resolve_normal", "on", triangles=_tri_all(_w_normals_opposed),
         note="normB = normC = -normA: the interpolation crosses 0 inside the triangle"),
    # the mesh, before the builders: corner C of the seen triangle, or every vertex
    Case("mesh-vertex-1e15", "mesh", "box_dst", "on", scene=_mesh(_m_add(1e15)), note="node bounds of 1e15; the faces at that vertex are about 1e15 |AB|, d about 1e16: finite"),
    Case("mesh-vertex-nan", "mesh", "leaf_root_box", "off", scene=_mesh(_m_component(0, NAN)), note="a NaN corner: the model is never filtered"),
    Case("mesh-vertex-3e19", "mesh", "bvh_build", "on", scene=_mesh(_m_set(3e19)), refused=_BUILDERS_REFUSE,
         note="refused where the builder has to split.  Where it builds (the FLAT bases' meshes are soups: the vertex is corner C of one "
              "triangle) the face is about 3e19 |AB| and d about 1e20: finite, the tables stay on"),
    Case("mesh-vertex-inf", "mesh", "bvh_build", "off", scene=_mesh(_m_component(1, INF)), refused={"bvh": "build_bvh"},
         note="refused where the builder has to split (bvh: a cube); many's target is a quad, one leaf like the FLAT bases' meshes, and builds"),
    Case("mesh-flat", "mesh", "box_dst", "on", scene=_mesh(_m_flat), note="every vertex's y = the first one's: flat boxes, 0 * inf in the slab test"),
    Case("mesh-point", "mesh", "box_dst", "on", scene=_mesh(_m_point), note="every vertex = the first"),
    Case("mesh-scale-1e-25", "mesh", "tri_eps", "on", scene=_mesh(_m_scale(1e-25)), note="the determinant underflows"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the side passes: every kind of object hazard (a sphere's radius and centre, a model's matrix records, every material field), >= 12
SIDE_CASES = ("radius-1e20", "radius-0", "radius-nan", "centre-nan", "centre-1e30", "model-position-nan", "matrix-singular", "matrix-scale-1e-20",
              "matrix-nan-entry", "smoothness-nan", "glass-ior-0", "glass-ior-nan", "emission-inf", "diffuse-nan", "glass-absorption-inf",
              # triangle and mesh values: ties, a face that is not finite, both normalisations, the threshold, a NaN and a flat box
              "tri-coincident", "tri-vertex-1e20", "tri-vertex-nan", "tri-normals-zero", "tri-normals-opposed", "tri-tiny-1e-4",
              "mesh-vertex-nan", "mesh-flat")
SIDE_BASES = ("flat-general", "bvh", "many")
# rt_nee_trace: the four emission and area hazards (a zero-radius emissive sphere and a singular emissive model are built by the test)
NEE_CASES = ("emission-inf", "emission-1e38", "radius-0", "matrix-singular")
# rt_nee_trace with the triangle model an emitter: the light table's area rule (S > 0 and finite, ng finite)
NEE_TRI_CASES = ("tri-degenerate", "tri-vertex-1e20", "tri-vertex-nan", "tri-tiny-1e-20")
# the device layouts that move and pre-difference the triangle records
LAYOUT_CASES, LAYOUT_BASES = ("tri-vertex-1e20", "tri-coincident", "mesh-vertex-nan"), ("bvh", "many")


def table(cases=CASES):
    """the catalogue as text: case x guard x tables x base scene"""
    rows = [f"{'case':38s} {'guard':18s} {'tables':6s} " + " ".join(f"{b:12s}" for b in BASES) + " marks"]
    for c in cases:
        marks = ", ".join(m for m, on in (("saturating", c.saturating), ("refused on " + " / ".join(c.refused or ()), c.refused is not None)) if on)
        rows.append(f"{c.name:38s} {c.guard:18s} {c.tables:6s} " +
                    " ".join(f"{'refused' if c.applies(b) and not c.builds(b) else 'x' if c.applies(b) else '-':12s}" for b in BASES) + " " + marks)
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
        if case is not None and case.kind in ("triangle", "mesh"):
            aim(pkg, base)
        if case is not None and case.scene:
            case.scene(pkg, sc, t)
        mgr = sc.make_manager(_NoTracer(), builder, w, h)
        mgr.renderSeed = seed
        self.base, self.case, self.w, self.h, self.targets = base, case, w, h, t
        self.meshes, self.bvh_quality = [m.Mesh for m in mgr.models], mgr.bvhQuality
        self.refused = None   # or (who, status): a builder's refusal, the named outcome of a (case, base) that does not build
        try:
            with np.errstate(all="ignore"):
                data = mgr.CreateAllMeshData(mgr.models)
        except pkg.abi.RtError as e:
            self.refused = ("build_bvh", e.status)
            return
        self.models, self.triangles, self.nodes = data["meshInfo"].copy(), data["triangles"], data["nodes"]
        self.tri_count = np.array([m.Mesh.triangle_count for m in mgr.models], dtype=np.int64)
        if case is not None and case.triangles:
            self.triangles = self.triangles.copy()
            case.triangles(pkg, self, t)
        self.spheres = mgr._pack_spheres()
        if case is not None and case.records:
            case.records(pkg, self.models, self.spheres, t)
        self.p = mgr.params()
        self.frame0 = 1
        if case is not None and case.params:
            case.params(self)
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


def _oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import __graft_entry__ as graft
    if "orc" not in _oracle.__dict__:
        _oracle.orc = graft.load_oracle()
    return _oracle.orc


def _mul_point(m, v, w):
    """rt_mul_point in fp32: row r = m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * w, summed left to right"""
    m, v = np.asarray(m, dtype=F32), np.asarray(v, dtype=F32)
    return np.stack([((m[r] * v[..., 0] + m[4 + r] * v[..., 1]) + m[8 + r] * v[..., 2]) + m[12 + r] * F32(w) for r in range(3)], axis=-1)


def hit_candidates(pkg, orc, rig, origins, dirs, hits=None):
    """-> (oracle_ray_collision's answers (n, 10), per ray the list of (model, index into rig.triangles) that can be its first hit, in
    model and buffer order).  The triangles are named the way tests/test_gpu_aov.py names one: over every model's range, those on which
    oracle_ray_triangle (the ray taken into the model's space with rt_mul_point's arithmetic, culling as RC:355) returns the hit's dst bit
    for bit.  More than one is a tie, which the walk order decides: coincident triangles, a ray through a shared edge.  A float64
    intersection of the same rays shortlists the triangles oracle_ray_triangle is asked about; a list is empty for a miss, a sphere, and
    a triangle the shortlist cannot reason about (a corner that is not finite).  (Models that share a mesh share triangle indices: the
    model says through which of them the triangle is seen.)"""
    F3 = C.c_float * 3
    n = len(origins)
    out10, out6, cands = (C.c_float * 10)(), (C.c_float * 6)(), [[] for _ in range(n)]
    if hits is None:   # (the caller may have asked the oracle already)
        ot = orc.create_tracer(1)
        try:
            rig.upload(ot)
            hits = np.zeros((n, 10), dtype=F32)
            for i in range(n):
                orc.ray_collision(ot.h, F3(*origins[i]), F3(*dirs[i]), out10)
                hits[i] = out10[:]
        finally:
            ot.close()
    rays = np.argwhere(hits[:, 0] != 0).ravel()
    for mi in range(len(rig.models) if len(rays) else 0):
        lo, cnt = int(rig.models["triOffset"][mi]), int(rig.tri_count[mi])
        T = rig.triangles[lo:lo + cnt]
        with np.errstate(all="ignore"):
            lo_ = _mul_point(rig.models["worldToLocal"][mi], origins[rays], 1)
            ld_ = _mul_point(rig.models["worldToLocal"][mi], dirs[rays], 0)
            # Moeller-Trumbore in float64, (rays, triangles): t close to the oracle's dst and inside the triangle with slack
            a, e1, e2 = (T["posA"].astype(np.float64), (T["posB"] - T["posA"]).astype(np.float64), (T["posC"] - T["posA"]).astype(np.float64))
            nrm = np.cross(e1, e2)
            o64, d64 = lo_.astype(np.float64), ld_.astype(np.float64)
            det = -(d64[:, None, :] * nrm[None]).sum(-1)
            ao = o64[:, None, :] - a[None]
            tt = (ao * nrm[None]).sum(-1) / det
            dao = np.cross(ao, d64[:, None, :])
            u, v = (e2[None] * dao).sum(-1) / det, -(e1[None] * dao).sum(-1) / det
            want = hits[rays, 2].astype(np.float64)[:, None]
            near = (np.abs(tt - want) <= 1e-3 * np.abs(want)) & (u >= -1e-3) & (v >= -1e-3) & (u + v <= 1 + 1e-3)
        cull = int(int(rig.models["material"]["flag"][mi]) != pkg.abi.MATERIAL_GLASS)
        for r, k in np.argwhere(near):   # (sorted by ray, then by triangle: buffer order)
            i = int(rays[r])
            orc.ray_triangle(F3(*lo_[r]), F3(*ld_[r]), T[k:k + 1].ctypes.data, cull, out6)
            if out6[0] != 0 and np.array([out6[2]], dtype=F32).view(np.uint32)[0] == hits[i:i + 1, 2].view(np.uint32)[0]:
                cands[i].append((mi, lo + int(k)))
    return hits, cands


def first_hit_triangles(pkg, orc, rig, origins, dirs):
    """(n, 2): the model and the index into rig.triangles of the triangle each ray hits first (of a tie, the first in buffer order),
    -1 = none"""
    _, cands = hit_candidates(pkg, orc, rig, origins, dirs)
    return np.array([c[0] if c else (-1, -1) for c in cands], dtype=np.int64).reshape(-1, 2)


EPS = F32(1e-8)   # RC:206's threshold


def threshold_edges():
    """{"below" / "at" / "above": (s1, s2)}: fp32 edge lengths near 1e-4 whose fp32 product is the float below 1E-8f, 1E-8f itself
    and the float above it, found by a search over the 81 x 81 neighbours of 1e-4f"""
    near = [F32(1e-4)]
    for _ in range(40):
        near = [np.nextafter(near[0], F32(0))] + near + [np.nextafter(near[-1], F32(1))]
    want = {"below": np.nextafter(EPS, F32(0)), "at": EPS, "above": np.nextafter(EPS, F32(1))}
    found = {}
    for x in near:
        for y in near:
            for k, v in want.items():
                if k not in found and F32(x * y) == v:
                    found[k] = (x, y)
    assert set(found) == set(want)
    return found


def threshold_rig(pkg, builder, base, s1, s2):
    """the base scene with model 0 (on every base an opaque model whose root box holds its local z axis) under identity matrices and every
    triangle of it A = (0, 0, z), B = (s1, 0, z), C = (0, s2, z): AB x AC = (0, 0, s1 * s2) without a rounding but the product's, and the
    determinant of the ray ((s1 / 4, s2 / 4, z + 0.01), (0, 0, -1)) is exactly fl(s1 * s2).  -> (rig, origin, direction)"""
    rig = Rig(pkg, builder, base)
    n = rig.nodes[int(rig.models["nodeOffset"][0])]
    assert (n["boundsMin"][:2] < 0).all() and (n["boundsMax"][:2] > 0).all() and int(rig.models["material"]["flag"][0]) != pkg.abi.MATERIAL_GLASS
    rig.models["localToWorld"][0] = rig.models["worldToLocal"][0] = _to_abi(np.eye(4))
    rig.triangles = rig.triangles.copy()
    T = rig.triangles[int(rig.models["triOffset"][0]):int(rig.models["triOffset"][0]) + int(rig.tri_count[0])]
    z = (n["boundsMin"][2] + n["boundsMax"][2]) / F32(2)   # (inside the root box, which the walk tests first; z - z = 0 all the same)
    T["posA"], T["posB"], T["posC"] = (0, 0, z), (s1, 0, z), (0, s2, z)
    for nrm in NORM:
        T[nrm] = (0, 0, 1)
    return rig, np.array([[s1 / F32(4), s2 / F32(4), z + F32(0.01)]], dtype=F32), np.array([[0, 0, -1]], dtype=F32)


_aimed = {}


def aim(pkg, base):
    """fills TARGETS[base]: tri_model, the seen triangle — the triangle that is, through that model, the first hit of the most pixel-centre
    rays of the unplanted scene — with its corners and its count, and most_seen, the (model, triangle, count) list of the whole scene,
    most seen first.  From the oracle, computed once."""
    t = TARGETS[base]
    if base not in _aimed:
        orc = _oracle()
        rig = Rig(pkg, orc, base)
        o, d = pixel_centre_rays(rig)
        first = first_hit_triangles(pkg, orc, rig, o.reshape(-1, 3), d.reshape(-1, 3))
        pairs, cnt = np.unique(first[first[:, 1] >= 0], axis=0, return_counts=True)
        order = np.lexsort((pairs[:, 1], pairs[:, 0], -cnt))
        most = [(int(pairs[k, 0]), int(pairs[k, 1]), int(cnt[k])) for k in order]

        def of(m):
            return [(i, c) for mi, i, c in most if mi == m]
        if t.tri_model is None:
            t.tri_model = t.model
            if not of(t.model) or of(t.model)[0][1] < SEEN_FLOOR:
                t.tri_model = most[0][0]
        mine = of(t.tri_model)
        assert mine, f"{base}: no pixel-centre ray hits model {t.tri_model} first"
        t.seen, t.seen_count = mine[0]
        t.seen_corners = np.stack([rig.triangles[p][t.seen] for p in POS]).copy()
        t.most_seen = most
        _aimed[base] = True
    return t


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
