"""The corrupted scenes of the validation fuzz, shared by tests/test_abi.py (through libraytrace_hip.so) and tests/test_scene_prep.py
(through the host-compiled, sanitized driver): one generator, so that both see the same arrays."""
import numpy as np


def scene_arrays(pkg, api, cfg=4, **kw):
    """The raw ABI arrays of a configuration: ({"meshInfo", "triangles", "nodes"}, spheres)"""
    sc = pkg.scenes.get(cfg, **kw)
    mgr = sc.make_manager(None, api)
    mgr.renderSeed = 1
    return mgr.CreateAllMeshData(mgr.models), mgr._pack_spheres()


def corrupted_scenes(data, seed=1, iterations=150):
    """Yields (iteration, kind, models, triangles, nodes): random child indices, triangle counts, bit flips in the node array, model
    offsets, links between subtrees, NaN / inf bounds — one to five of one kind per scene, all drawn from ONE seeded stream."""
    rng = np.random.default_rng(seed)
    for it in range(iterations):
        nodes, models, tris = data["nodes"].copy(), data["meshInfo"].copy(), data["triangles"]
        kind = it % 6
        for _ in range(int(rng.integers(1, 6))):
            i = int(rng.integers(0, len(nodes)))
            if kind == 0:
                nodes[i]["startIndex"] = int(rng.integers(-5, len(nodes) + 5))
            elif kind == 1:
                nodes[i]["triangleCount"] = int(rng.integers(-3, 200))
            elif kind == 2:
                raw = nodes.view(np.uint8)
                raw[int(rng.integers(0, raw.size))] ^= np.uint8(1 << int(rng.integers(0, 8)))
            elif kind == 3:
                m = int(rng.integers(0, len(models)))
                models[m]["nodeOffset"] = int(rng.integers(-2, len(nodes) + 2))
                models[m]["triOffset"] = int(rng.integers(-2, len(tris) + 2))
            elif kind == 4:
                nodes[i]["startIndex"] = nodes[int(rng.integers(0, len(nodes)))]["startIndex"]
            else:
                nodes[i]["boundsMin"][int(rng.integers(0, 3))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
        yield it, kind, models, tris, nodes
