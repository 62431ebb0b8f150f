"""The seeded scenes of tests/test_gpu_fuzz.py that other tests render too."""
import numpy as np


def random_scene(pkg, seed):
    rng = np.random.default_rng(seed)
    M, T = pkg.RayTracingMaterial, pkg.Transform
    meshes = [pkg.meshes.cube(), pkg.meshes.quad(), pkg.meshes.rounded_cube(4), pkg.meshes.icosphere(2, 1.0, int(seed))]

    def material():
        flag = int(rng.choice([0, 0, 1, 2]))
        return M(flag=flag, diffuseCol=tuple(rng.uniform(0.05, 1, 3)) + (1,), emissionCol=tuple(rng.uniform(0, 1, 3)) + (1,),
                 specularCol=tuple(rng.uniform(0.3, 1, 3)) + (1,), absorption=tuple(rng.uniform(0, 1, 3)) + (1,),
                 absorptionMultiplier=float(rng.uniform(0, 2)), emissionStrength=float(rng.choice([0, 0, 0, 4.0])),
                 smoothness=float(rng.uniform(0, 1)), specularProbability=float(rng.uniform(0, 1)),
                 ior=float(rng.uniform(1.0, 2.2)))
    spheres = [pkg.Sphere(tuple(rng.uniform(-3, 3, 3) + [0, 1, 3]), float(rng.uniform(0.2, 1.2)), material())
               for _ in range(int(rng.integers(0, 21)))]
    models = []
    for _ in range(int(rng.integers(0, 9))):
        scale = tuple(rng.uniform(0.3, 2.5, 3)) if rng.random() < 0.5 else float(rng.uniform(0.3, 2.0))
        models.append(pkg.Model(meshes[int(rng.integers(0, 4))], material(),
                                T(tuple(rng.uniform(-3, 3, 3) + [0, 1, 3]), tuple(rng.uniform(0, 360, 3)), scale)))
    if rng.random() < 0.6:  # a big ground quad
        models.append(pkg.Model(meshes[1], material(), T((0, -0.5, 3), (90, 0, 0), (30, 30, 1))))
    cam = pkg.Camera(T(tuple(rng.uniform(-1, 1, 3) + [0, 1, -5]), (float(rng.uniform(-10, 15)), float(rng.uniform(-15, 15)), 0)),
                     fieldOfView=float(rng.uniform(30, 90)))
    settings = dict(maxBounceCount=int(rng.integers(0, 13)), numRaysPerPixel=int(rng.integers(1, 5)),
                    divergeStrength=float(rng.uniform(0, 3)), defocusStrength=float(rng.choice([0, 0, 50, 200])),
                    focusDistance=float(rng.uniform(0.5, 8)), useSky=bool(rng.random() < 0.7), sunFocus=float(rng.uniform(100, 900)),
                    sunIntensity=float(rng.uniform(1, 20)), accumulate=True,
                    bvhQuality=int(rng.choice([0, 1, 1, 2])))
    w, h = int(rng.integers(17, 70)), int(rng.integers(9, 40))
    frames = int(rng.integers(1, 4))
    sc = pkg.scenes.SceneDescription(f"fuzz{seed}", w, h, frames, settings, cam, models, spheres)
    return sc, int(rng.integers(-2**31, 2**31 - 1))


def crowded_overflow_scene(pkg, n_models, n_spheres, seed=7):
    """More models than the 64-bit root-filter mask holds and more spheres than one 32-wide
    candidate word: the kernel's overflow paths (models >= 64 visited unfiltered, second sphere
    word) must give the reference's in-order results."""
    rng = np.random.default_rng(seed)
    M, T = pkg.RayTracingMaterial, pkg.Transform
    meshes = [pkg.meshes.cube(), pkg.meshes.rounded_cube(3), pkg.meshes.quad()]
    models = [pkg.Model(meshes[i % 3], M(flag=int(i % 4 == 3) * 2, diffuseCol=tuple(rng.uniform(0.2, 1, 3)) + (1,), ior=1.4,
                                         emissionStrength=float(i % 9 == 0) * 3.0, emissionCol=(1, 0.9, 0.7, 1)),
                        T(tuple(rng.uniform(-4, 4, 3) + [0, 1.5, 4]), tuple(rng.uniform(0, 360, 3)), float(rng.uniform(0.2, 0.7))))
              for i in range(n_models)]
    spheres = [pkg.Sphere(tuple(rng.uniform(-4, 4, 3) + [0, 1.5, 4]), float(rng.uniform(0.1, 0.5)),
                          M(flag=int(i % 5 == 0) * 2, diffuseCol=tuple(rng.uniform(0.2, 1, 3)) + (1,), ior=1.5, smoothness=0.6,
                            specularProbability=0.4))
               for i in range(n_spheres)]
    cam = pkg.Camera(T((0, 1.5, -6), (0, 0, 0)), fieldOfView=55.0)
    settings = dict(maxBounceCount=5, numRaysPerPixel=2, divergeStrength=0.5, useSky=True, accumulate=True, bvhQuality=1)
    return pkg.scenes.SceneDescription("crowded", 88, 48, 2, settings, cam, models, spheres)
