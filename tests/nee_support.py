"""What the tests of rt_nee_trace (tests/test_gpu_nee.py) share with those of rt_mis_trace: the scenes' arrays (built once per name and
process, shared, never written), the 200 camera rays, tracers and comparisons."""
import numpy as np

import nee_reference as nr
import query_support as tq
import radiance_reference as rr

F = np.float32
FRAME = 3
W, H = 20, 10  # 200 camera rays: three blocks and a partial one
LAYOUTS = ["dense", "pre", "pre,align", "pre,arena", "pre,arena,cache", "pre,hot=2,arena,palign"]
_SCENES = {}


class SceneArrays:
    """A scene description's arrays as rt_upload_scene takes them (tests/query_support.py's Scene for descriptions it does not know)."""

    def __init__(self, api, desc):
        self.desc = desc
        mgr = desc.make_manager(None, api, 64, 36)
        data = mgr.CreateAllMeshData(mgr.models)
        self.models, self.triangles, self.nodes = data["meshInfo"], data["triangles"], data["nodes"]
        self.spheres = mgr._pack_spheres()

    def upload(self, tracer, models=None, spheres=None):
        tracer.upload_scene(self.models if models is None else models, self.triangles, self.nodes, self.spheres if spheres is None else spheres)
        return tracer

    def stripped(self):
        """The arrays with every emitter put out: emissionStrength 0 (a checkered material's second colour stays)."""
        models, spheres = self.models.copy(), self.spheres.copy()
        models["material"]["emissionStrength"] = 0
        spheres["material"]["emissionStrength"] = 0
        return models, spheres


def describe(pkg, name):
    if name == "crowded70_emissive":  # the MANY variant: model 0 (the cube at the origin, a ball poking through its faces) and sphere 1 made emissive
        d = tq.crowded_identity_scene(pkg)
        M = pkg.RayTracingMaterial
        d.models[0].material = M(diffuseCol=(0, 0, 0, 1), emissionCol=(1, 0.8, 0.5, 1), emissionStrength=12.0)
        d.spheres[1].material = M(diffuseCol=(0.2, 0.2, 0.2, 1), emissionCol=(0.4, 0.6, 1, 1), emissionStrength=5.0)
        return d
    if name.startswith("nee_"):
        return nr.build_scene(pkg, name)
    return tq.scene_of(pkg, name)


def scene(pkg, api, name):
    if name not in _SCENES:
        _SCENES[name] = SceneArrays(api, describe(pkg, name))
    return _SCENES[name]


def hip_tracer(api, sc, p, **arrays):
    tr = sc.upload(api.create_tracer(0), **arrays)
    tr.set_params(p)
    return tr


def camera_batch(pkg, api, orc, sc, w, h, bounce):
    tweak = dict(rr.NO_DOF, numRaysPerPixel=1)
    if bounce is not None:
        tweak["maxBounceCount"] = bounce
    p = rr.params_of(sc, api, w, h, tweak)
    origins, dirs, states = rr.camera_rays(orc, p, w, h, FRAME)
    return p, pkg.abi.make_path_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3), states.reshape(-1))


def assert_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    rr.assert_rgb(got["rgb"], want["rgb"], what)
    bad = np.argwhere(got["rng"] != want["rng"]).ravel()
    assert not len(bad), f"{what}: rng of {len(bad)} rays differs; first is ray {bad[0]}"


def chained(call, ray, chains, rounds):
    """chains x rounds samples of one ray: `chains` generator sequences, each chained through `rounds` calls."""
    rays = np.repeat(ray, chains)
    rays["rng"] = (np.arange(chains, dtype=np.uint64) * 2654435761 + 12345) % (1 << 32)
    out = np.zeros((rounds, chains, 3), dtype=F)
    for k in range(rounds):
        rec = call(rays)
        out[k] = rec["rgb"]
        rays["rng"] = rec["rng"]
    return out.reshape(-1, 3)


def grid_mesh(pkg, nx=256, ny=128):
    """nx x ny quads in the plane z = 0, two triangles each (2^16 at the default), front side -z like the Quad."""
    xs, ys = np.meshgrid(np.linspace(-0.5, 0.5, nx + 1), np.linspace(-0.5, 0.5, ny + 1), indexing="xy")
    verts = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], axis=1).astype(F)
    i = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    a, b, c, d = i, i + 1, i + nx + 1, i + nx + 2  # the Quad's corners 0, 1, 2, 3 and its triangles (0, 3, 1), (3, 0, 2)
    idx = np.stack([a, d, b, d, a, c], axis=1).ravel().astype(np.int32)
    return pkg.meshes.Mesh(verts, np.tile(np.array([[0, 0, -1]], dtype=F), (len(verts), 1)), idx, "Grid")


def without_cache(layout):
    """tests/test_layout.py's: `used` reports the records the cache really holds, so the cache word is compared apart"""
    return ",".join(w for w in layout.split(",") if not w.startswith("cache")) or "dense"
