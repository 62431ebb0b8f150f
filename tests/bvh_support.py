"""The meshes the BVH builder is tested on (tests/test_bvh.py), for the tests that pin the reference's builder to the same cases."""
import numpy as np


def mesh_cases(pkg):
    m = pkg.meshes
    rng = np.random.default_rng(7)
    # triangle soup: overlapping random triangles (ragged leaves, SAH refusing splits)
    v = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    soup = m.Mesh(v, np.tile([[0, 1, 0]], (300, 1)), rng.integers(0, 300, 3 * 500).astype(np.int32), "soup")
    # degenerate: every triangle identical (all centroids equal -> single leaf > 127 triangles)
    same = m.Mesh(v[:3], np.tile([[0, 1, 0]], (3, 1)), np.tile([0, 1, 2], 200).astype(np.int32), "same")
    # flat mesh in the y=0 plane (a zero-size axis: NaN in CeilToInt(axisSize/maxAxis*K) cannot occur, 0 can)
    flat_v = np.stack([rng.uniform(-1, 1, 200), np.zeros(200), rng.uniform(-1, 1, 200)], axis=1).astype(np.float32)
    flat = m.Mesh(flat_v, np.tile([[0, 1, 0]], (200, 1)), rng.integers(0, 200, 3 * 150).astype(np.int32), "flat")
    # a single point (all sizes 0 -> 0/0 NaN in the split count)
    point = m.Mesh(np.zeros((3, 3), np.float32), np.tile([[0, 1, 0]], (3, 1)), np.tile([0, 1, 2], 12).astype(np.int32), "point")
    one = m.Mesh(v[:3], np.tile([[0, 1, 0]], (3, 1)), np.array([0, 1, 2], np.int32), "one")
    return [m.quad(), m.cube(), m.rounded_cube(6), m.icosphere(3), m.icosphere(3, 1.0, 4), soup, same, flat, point, one]
